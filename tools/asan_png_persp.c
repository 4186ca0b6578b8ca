/* DEVELOPMENT / TEST TOOLING: the host side of the perspective warp (debig_png_persp_quantise, debig_png_persp_range,
 * debig_png_decode_batch_tensor_persp, _labels_persp, _color_labels_persp) under AddressSanitizer and UBSan, as a stand-alone CPU
 * program (tools/asan_png_persp.sh builds and runs it; no GPU, no Python).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called: everything driven here -- the quantiser and the range check at their limits, the
 * argument checks, and the statuses decided when IHDR has been read (E_LABEL > E_BOX > E_WARP > what comes later in the file) --
 * is decided on the host, before any device is looked for.  The files are a signature and an IHDR chunk with nothing behind. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "decode_png.h"

#define SENTINEL 0xABCDu
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

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
static uint32_t status[N], unmatched[N];
static debig_png_persp persps[N];
static void *const OUT = (void *)(uintptr_t)0x10000;

static void reset(void)
{
    for (uint32_t i = 0; i < N; i++) status[i] = unmatched[i] = SENTINEL;
}

static void untouched(int rc)
{
    CHECK(rc == DEBIG_PNG_BAD_ARG);
    for (uint32_t i = 0; i < N; i++) CHECK(status[i] == SENTINEL && unmatched[i] == SENTINEL);
}

static void identity(double *m)
{
    const double id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memcpy(m, id, sizeof id);
}

int main(void)
{
    /* ---- the quantiser and the range check */
    int64_t m[9];
    double M[9];
    identity(M);
    CHECK(debig_png_persp_quantise(M, m) == 1 && m[0] == 65536 && m[4] == 65536 && m[8] == ((int64_t)1 << 30) && m[6] == 0);
    M[6] = 4.0; M[7] = -4.0; M[8] = 0.5 / 1073741824.0;
    CHECK(debig_png_persp_quantise(M, m) == 1 && m[6] == ((int64_t)1 << 32) && m[7] == -((int64_t)1 << 32) && m[8] == 1);
    M[8] = -1.5 / 1073741824.0;
    CHECK(debig_png_persp_quantise(M, m) == 1 && m[8] == -2);
    const double bad[5] = {NAN, INFINITY, -INFINITY, nextafter(4.0, 5.0), -nextafter(4.0, 5.0)};
    for (uint32_t k = 0; k < 9; k++)
        for (uint32_t b = 0; b < 5; b++) {
            identity(M);
            M[k] = k < 6 && b >= 3 ? (k == 2 || k == 5 ? 16777216.0 : 32768.0) * (b == 3 ? 1.0 : -1.0) * (1.0 + 1e-12) : bad[b];
            CHECK(debig_png_persp_quantise(M, m) == 0);
        }
    /* D == 2^21 and D == 2^33 - 1 at a corner pass, one less and one more do not; sizes and p[] beyond their limits do not */
    int64_t r[9] = {0, 0, 0, 0, 0, 0, 0, 0, (int64_t)1 << 20};
    CHECK(debig_png_persp_range(r, 16384, 16384) == 1);
    r[6] = 1; r[8] = ((int64_t)1 << 20) - 1;                       /* D(0, 0) = 2^21 - 1, the smallest */
    CHECK(debig_png_persp_range(r, 9, 5) == 0);
    r[8] = (int64_t)1 << 20;                                        /* 2^21 + 1 */
    CHECK(debig_png_persp_range(r, 9, 5) == 1);
    r[6] = 1; r[8] = ((int64_t)1 << 32) - 9;                        /* D at the last column: 17 + 2^33 - 18 = 2^33 - 1 */
    CHECK(debig_png_persp_range(r, 9, 5) == 1);
    r[8]++;
    CHECK(debig_png_persp_range(r, 9, 5) == 0);
    r[6] = 0; r[7] = -1; r[8] = ((int64_t)1 << 20) + 5;             /* D at the last row: -9 + 2^21 + 10 = 2^21 + 1 */
    CHECK(debig_png_persp_range(r, 9, 5) == 1);
    r[8]--;
    CHECK(debig_png_persp_range(r, 9, 5) == 0);
    r[7] = 0; r[8] = (int64_t)1 << 30;
    CHECK(debig_png_persp_range(r, 0, 5) == 0 && debig_png_persp_range(r, 9, 16385) == 0 && debig_png_persp_range(r, 1, 1) == 1);
    r[6] = ((int64_t)1 << 32) + 1; r[8] = -((int64_t)1 << 31);
    CHECK(debig_png_persp_range(r, 2, 2) == 0);
    r[6] = INT64_MIN; r[7] = INT64_MAX; r[8] = INT64_MAX;            /* nothing is multiplied before the limits are checked */
    CHECK(debig_png_persp_range(r, 16384, 16384) == 0);

    /* ---- the calls.  Heap copies of exactly the files' sizes: a read past their end is ASan's to see */
    uint8_t tmp[64];
    const struct { uint32_t w, h; uint8_t depth, ct; } spec[N] = {{9, 7, 16, 2}, {9, 7, 8, 2}, {9, 7, 8, 3}, {9, 7, 4, 0}, {9, 7, 8, 0}};
    for (uint32_t i = 0; i < N; i++) {
        sizes[i] = stub_png(tmp, spec[i].w, spec[i].h, spec[i].depth, spec[i].ct);
        files[i] = (uint8_t *)malloc(sizes[i]);
        memcpy(files[i], tmp, sizes[i]);
        identity(persps[i].m);
    }
    const uint8_t *const *in = (const uint8_t *const *)files;

    debig_png_tensor_desc td;
    memset(&td, 0, sizeof td);
    td.out_w = 8; td.out_h = 6; td.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8; td.dtype = DEBIG_PNG_T_F32;
    for (uint32_t k = 0; k < 4; k++) td.scale[k] = 1.0f;
    debig_png_warp_desc wd;
    memset(&wd, 0, sizeof wd);
    debig_png_color colors[N];
    debig_png_tone tones[N];
    debig_png_blur blurs[N];
    memset(colors, 0, sizeof colors);
    memset(tones, 0, sizeof tones);
    memset(blurs, 0, sizeof blurs);

    /* the tensor call's argument checks, through each of the four affine calls it stands for */
    for (uint32_t v = 0; v < 5; v++) { /* (and the blur call with blurs alone) */
        const debig_png_color *cs = v == 1 || v == 3 ? colors : NULL;
        const debig_png_tone *ts = v == 2 || v == 3 ? tones : NULL;
        const debig_png_blur *bs = v >= 3 ? blurs : NULL;
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, NULL, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, &wd));
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, NULL));
        /* neither the maps nor their descriptor, with tones or blurs as well: never a decode without a map */
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, NULL, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, NULL));
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, NULL, &wd));
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, NULL, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, &wd));
        wd.filter = DEBIG_PNG_FILTER_BICUBIC;
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, &wd));
        wd.filter = DEBIG_PNG_FILTER_BILINEAR; wd.border_mode = 2;
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, &wd));
        wd.border_mode = DEBIG_PNG_BORDER_CONSTANT; wd.border[1] = 256;
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, &wd));
        wd.border[1] = 255; wd.alpha_mode = 1;
        reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 0, bs, status, NULL, N, 0, &td, &wd));
        wd.alpha_mode = 0;
        if (ts || bs) { /* tables counted but not given */
            reset(); untouched(debig_png_decode_batch_tensor_persp(in, sizes, OUT, NULL, persps, cs, ts, NULL, 2, bs, status, NULL, N, 0, &td, &wd));
        }
    }
    CHECK(debig_png_decode_batch_tensor_persp(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, 0, NULL, NULL) == 0);

    /* the statuses decided at IHDR: a bad box ahead of a bad map; NaN, an entry beyond 4, a horizon through the output, a map whose
     * D only just leaves the range at one corner -- each ahead of the missing IDAT; a good map leaves what the file lacks */
    const debig_png_box boxes[N] = {{0, 0, 10, 1}, {0, 0, 0, 0}, {1, 1, 8, 6}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    persps[0].m[7] = NAN;
    persps[1].m[6] = 4.5;
    persps[2].m[6] = -0.25;                         /* D = 1 - 0.25 (X + 1/2): zero at X = 3.5 */
    persps[3].m[7] = -1.0 / 5.5;                    /* D = 0 at the last row of the 8 x 6 output */
    for (uint32_t v = 0; v < 3; v++) {
        reset();
        CHECK(debig_png_decode_batch_tensor_persp(in, sizes, OUT, boxes, persps, v == 1 ? colors : NULL, v == 2 ? tones : NULL, NULL, 0,
                                                  v == 2 ? blurs : NULL, status, NULL, N, 0, &td, &wd) == 0);
        CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
        CHECK(status[4] != 0 && status[4] != SENTINEL && status[4] != DEBIG_PNG_E_WARP);
    }

    debig_png_label_desc ld;
    memset(&ld, 0, sizeof ld);
    ld.out_w = 8; ld.out_h = 6; ld.dtype = DEBIG_PNG_L_I32;
    debig_png_label_warp_desc lw = {DEBIG_PNG_BORDER_CONSTANT, -1};
    reset(); untouched(debig_png_decode_batch_labels_persp(in, sizes, OUT, NULL, NULL, status, NULL, N, 0, &ld, &lw));
    reset(); untouched(debig_png_decode_batch_labels_persp(in, sizes, OUT, NULL, persps, status, NULL, N, 0, &ld, NULL));
    lw.border_mode = 2;
    reset(); untouched(debig_png_decode_batch_labels_persp(in, sizes, OUT, NULL, persps, status, NULL, N, 0, &ld, &lw));
    lw.border_mode = DEBIG_PNG_BORDER_CONSTANT;
    ld.dtype = DEBIG_PNG_L_U8;
    reset(); untouched(debig_png_decode_batch_labels_persp(in, sizes, OUT, NULL, persps, status, NULL, N, 0, &ld, &lw));
    ld.dtype = DEBIG_PNG_L_I32;
    reset();
    CHECK(debig_png_decode_batch_labels_persp(in, sizes, OUT, boxes, persps, status, NULL, N, 0, &ld, &lw) == 0);
    CHECK(status[0] == DEBIG_PNG_E_LABEL && status[1] == DEBIG_PNG_E_LABEL && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
    CHECK(status[4] != 0 && status[4] != SENTINEL && status[4] != DEBIG_PNG_E_WARP);
    CHECK(debig_png_decode_batch_labels_persp(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) == 0);

    uint32_t keys[3] = {1, 2, 3};
    int32_t values[3] = {4, 5, 6};
    debig_png_color_map map = {3, 0, keys, values};
    debig_png_color_label_desc cd = {8, 6, DEBIG_PNG_L_I32, DEBIG_PNG_CL_MAP, -1, 1, &map, 0, 0};
    reset(); untouched(debig_png_decode_batch_color_labels_persp(in, sizes, OUT, NULL, NULL, status, NULL, unmatched, N, 0, &cd, &lw));
    reset(); untouched(debig_png_decode_batch_color_labels_persp(in, sizes, OUT, NULL, persps, status, NULL, unmatched, N, 0, &cd, NULL));
    cd.n_maps = 2; /* an inherited check, found after a table has been made */
    reset(); untouched(debig_png_decode_batch_color_labels_persp(in, sizes, OUT, NULL, persps, status, NULL, unmatched, N, 0, &cd, &lw));
    cd.n_maps = 1;
    reset();
    CHECK(debig_png_decode_batch_color_labels_persp(in, sizes, OUT, boxes, persps, status, NULL, unmatched, N, 0, &cd, &lw) == 0);
    CHECK(status[0] == DEBIG_PNG_E_LABEL && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
    CHECK(status[4] != 0 && status[4] != SENTINEL && status[4] != DEBIG_PNG_E_WARP);
    for (uint32_t i = 0; i < N; i++) CHECK(unmatched[i] == 0);
    CHECK(debig_png_decode_batch_color_labels_persp(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) == 0);

    for (uint32_t i = 0; i < N; i++) free(files[i]);
    puts("asan_png_persp: all checks passed");
    return 0;
}
