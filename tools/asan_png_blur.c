/* DEVELOPMENT / TEST TOOLING: the host side of debig_png_decode_batch_tensor_blur under AddressSanitizer and UBSan, as a
 * stand-alone CPU program (tools/asan_png_blur.sh builds and runs it; no GPU, no Python).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called: everything driven here -- debig_png_blur_weights, the argument checks and the statuses
 * decided when IHDR has been read (E_BOX > E_WARP > E_COLOR > E_TONE > E_BLUR > what comes later in the file) -- is decided on the
 * host, before any device is looked for.  The files are a signature and an IHDR chunk with nothing behind them. */
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

#define N 6
static uint8_t *files[N];
static uint64_t sizes[N];
static uint32_t status[N];
static debig_png_warp warps[N];
static debig_png_color colors[N];
static debig_png_tone tones[N];
static debig_png_blur blurs[N];
static void *const OUT = (void *)(uintptr_t)0x10000; /* never dereferenced */

static int call(const debig_png_tensor_desc *d, const debig_png_warp *ws, const debig_png_color *cs, const debig_png_tone *ts,
                const debig_png_blur *bs, const debig_png_alpha_desc *ad, const debig_png_filter_desc *fd,
                const debig_png_warp_desc *wd, const debig_png_box *bx)
{
    for (uint32_t i = 0; i < N; i++) status[i] = SENTINEL;
    return debig_png_decode_batch_tensor_blur((const uint8_t *const *)files, sizes, OUT, bx, ws, cs, ts, NULL, 0, bs, status, NULL, N, 0,
                                              d, ad, fd, wd);
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

    /* ---- the weights helper: a heap buffer of exactly 63 taps */
    int16_t *q = (int16_t *)malloc(63 * sizeof(int16_t));
    CHECK(q);
    const double sigmas[] = {5e-324, 1e-3, 0.1, 0.8, 2.0, 3.7, 10.0, 30.0, 999.0, 1000.0};
    for (uint32_t ksize = 3; ksize <= 63; ksize += 2) {
        for (uint32_t s = 0; s < sizeof sigmas / sizeof *sigmas; s++) {
            memset(q, 0x5A, 63 * sizeof(int16_t));
            CHECK(debig_png_blur_weights(ksize, sigmas[s], q) == 1);
            int32_t sum = 0;
            for (uint32_t j = 0; j < 63; j++) {
                CHECK(q[j] >= 0 && (j < ksize || q[j] == 0));
                if (j < ksize) CHECK(q[j] == q[ksize - 1 - j]);
                sum += q[j];
            }
            CHECK(sum == 16384);
        }
    }
    CHECK(debig_png_blur_weights(3, 0.1, q) == 1 && q[0] == 0 && q[1] == 16384 && q[2] == 0);
    const uint32_t bad_k[] = {0, 1, 2, 4, 62, 64, 65, 0xFFFFFFFFu};
    for (uint32_t k = 0; k < sizeof bad_k / sizeof *bad_k; k++) CHECK(debig_png_blur_weights(bad_k[k], 1.0, q) == 0);
    const double bad_s[] = {0.0, -0.0, -1.0, 1000.5, 1e300, INFINITY, -INFINITY, NAN};
    for (uint32_t s = 0; s < sizeof bad_s / sizeof *bad_s; s++) CHECK(debig_png_blur_weights(23, bad_s[s], q) == 0);
    free(q);

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
    untouched(call(&d, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));   /* blurs NULL */
    untouched(call(&d, NULL, NULL, tones, NULL, NULL, NULL, NULL, NULL));  /* blurs NULL, tones given */
    for (uint32_t i = 0; i < N; i++) status[i] = SENTINEL;
    CHECK(debig_png_decode_batch_tensor_blur((const uint8_t *const *)files, sizes, OUT, NULL, NULL, NULL, tones, NULL, 1, blurs, status,
                                             NULL, N, 0, &d, NULL, NULL, NULL) == DEBIG_PNG_BAD_ARG && status[0] == SENTINEL); /* tables */
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_16;
    untouched(call(&d, NULL, NULL, NULL, blurs, NULL, NULL, NULL, NULL));  /* 16 bits */
    d.out_format = DEBIG_PNG_FMT_RGBA | DEBIG_PNG_FMT_8;
    ad.mode = DEBIG_PNG_ALPHA_PREMULTIPLIED;
    untouched(call(&d, NULL, NULL, NULL, blurs, &ad, NULL, NULL, NULL));   /* PREMULTIPLIED */
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8;
    ad.mode = DEBIG_PNG_ALPHA_OVER;
    untouched(call(&d, NULL, colors, NULL, blurs, &ad, NULL, NULL, NULL)); /* alpha with a matrix */
    untouched(call(&d, NULL, colors, tones, blurs, NULL, &fd, NULL, NULL)); /* BICUBIC with a matrix */
    untouched(call(&d, warps, NULL, NULL, blurs, NULL, NULL, NULL, NULL)); /* warps without their descriptor */
    untouched(call(&d, NULL, NULL, NULL, blurs, NULL, NULL, &wd, NULL));   /* the descriptor without warps */
    untouched(call(&d, warps, NULL, NULL, blurs, NULL, &fd, &wd, NULL));   /* a filter descriptor under a warp */
    untouched(call(NULL, NULL, NULL, NULL, blurs, NULL, NULL, NULL, NULL));
    d.out_format = DEBIG_PNG_FMT_NATIVE;
    CHECK(call(&d, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == DEBIG_PNG_BAD_FORMAT && status[0] == SENTINEL);
    CHECK(debig_png_decode_batch_tensor_blur(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL,
                                             NULL) == 0);

    /* ---- the order of the statuses decided at IHDR: E_BOX > E_WARP > E_COLOR > E_TONE > E_BLUR > what the file holds later (here:
     * nothing) */
    const debig_png_box boxes[N] = {{0, 0, 10, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    warps[0].m[2] = NAN;
    warps[1].m[0] = 32769.0;
    colors[0].m[5] = colors[1].m[6] = colors[2].m[7] = NAN;
    const debig_png_tone badt[N] = {{DEBIG_PNG_TONE_POSTERIZE, 9}, {7, 0}, {DEBIG_PNG_TONE_EQUALIZE, 1}, {DEBIG_PNG_TONE_SOLARIZE, 257},
                                    {DEBIG_PNG_TONE_EQUALIZE, 0}, {DEBIG_PNG_TONE_NONE, 0}};
    const debig_png_blur badb[N] = {{DEBIG_PNG_BLUR_GAUSSIAN, 4, 1.0}, {3, 3, 1.0}, {DEBIG_PNG_BLUR_SHARPNESS, 0, NAN},
                                    {DEBIG_PNG_BLUR_GAUSSIAN, 3, 0.0}, {DEBIG_PNG_BLUR_SHARPNESS, 0, -16.5}, {DEBIG_PNG_BLUR_GAUSSIAN, 63, 1000.0}};
    d.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8;
    CHECK(call(&d, warps, colors, badt, badb, NULL, NULL, &wd, boxes) == 0);
    CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_COLOR && status[3] == DEBIG_PNG_E_TONE &&
          status[4] == DEBIG_PNG_E_BLUR);
    CHECK(status[5] != DEBIG_PNG_OK && status[5] != DEBIG_PNG_E_BLUR && status[5] != SENTINEL); /* the file ends behind IHDR */
    const uint32_t later = status[5];
    CHECK(call(&d, NULL, colors, badt, badb, NULL, NULL, NULL, boxes) == 0);
    CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_COLOR && status[2] == DEBIG_PNG_E_COLOR && status[3] == DEBIG_PNG_E_TONE &&
          status[4] == DEBIG_PNG_E_BLUR && status[5] == later);
    d.resize_flags = DEBIG_PNG_RESIZE_ANTIALIAS;
    d.out_format = DEBIG_PNG_FMT_GRAY | DEBIG_PNG_FMT_8;
    CHECK(call(&d, NULL, NULL, NULL, badb, &ad, &fd, NULL, boxes) == 0); /* tones NULL */
    CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_BLUR && status[2] == DEBIG_PNG_E_BLUR && status[3] == DEBIG_PNG_E_BLUR &&
          status[4] == DEBIG_PNG_E_BLUR && status[5] == later);
    for (uint32_t i = 0; i < N; i++) free(files[i]);
    puts("asan_png_blur: ok");
    return 0;
}
