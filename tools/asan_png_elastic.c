/* DEVELOPMENT / TEST TOOLING: the host side of the elastic deformation (debig_png_elastic_quantise, _cell, _weights, _displacement,
 * debig_png_decode_batch_tensor_elastic, _labels_elastic, _color_labels_elastic) under AddressSanitizer and UBSan, as a stand-alone
 * CPU program (tools/asan_png_elastic.sh builds and runs it; no GPU, no Python).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called: everything driven here -- the quantiser at its limits, the helpers over every t and at
 * the largest grid, nodes and sizes (UBSan watches the 64-bit sums and the shifts), the argument checks, and the statuses decided
 * when IHDR has been read (E_LABEL > E_BOX > E_WARP > what comes later in the file) -- is decided on the host, before any device
 * is looked for.  The files are a signature and an IHDR chunk with nothing behind; the fields are heap copies of exactly
 * grid_h x grid_w x 2 doubles, so a read past a field's end is ASan's to see. */
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
#define GW 5u
#define GH 3u
static uint8_t *files[N];
static uint64_t sizes[N];
static uint32_t status[N], unmatched[N];
static debig_png_warp warps[N];
static debig_png_elastic elastics[N];
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

int main(void)
{
    /* ---- the quantiser */
    int32_t q[6];
    const double v[6] = {4096.0, -4096.0, 0.5 / 65536.0, -0.5 / 65536.0, 1.49999 / 65536.0, -0.0};
    CHECK(debig_png_elastic_quantise(v, 6, q) == 1 && q[0] == (1 << 28) && q[1] == -(1 << 28) && q[2] == 1 && q[3] == -1 && q[4] == 1 && q[5] == 0);
    const double bad[6] = {NAN, INFINITY, -INFINITY, nextafter(4096.0, 5000.0), -nextafter(4096.0, 5000.0), 1e300};
    for (uint32_t b = 0; b < 6; b++) {
        double w[3] = {1.0, bad[b], 2.0};
        CHECK(debig_png_elastic_quantise(w, 3, q) == 0);
    }
    CHECK(debig_png_elastic_quantise(v, 0, q) == 1);

    /* ---- the weights over every t, the cells at the ends of the largest axis */
    for (uint32_t t = 0; t <= 16384; t++) {
        int32_t w[4];
        debig_png_elastic_weights(t, w);
        CHECK(w[0] + w[1] + w[2] + w[3] == 16384);
        CHECK(abs(w[0]) + abs(w[1]) + abs(w[2]) + abs(w[3]) <= 20480);
    }
    uint32_t k, t;
    debig_png_elastic_cell(16383, 16384, 33, &k, &t);
    CHECK(k == 31 && t <= 16384);
    debig_png_elastic_cell(0, 1, 33, &k, &t);
    CHECK(k == 16 && t == 0);
    debig_png_elastic_cell(0, 16384, 2, &k, &t);
    CHECK(k == 0 && t == 1);

    /* ---- the displacement: every node at the limit with alternating signs, the largest grid, every pixel of a 64 x 257 output and
     * the corners of a 16384 x 16384 one; heap copies of exactly the grid's size */
    int32_t *g = (int32_t *)malloc(33u * 33u * 2u * sizeof(int32_t));
    for (uint32_t i = 0; i < 33u * 33u; i++) {
        g[2 * i] = i % 2 ? -(1 << 28) : (1 << 28);
        g[2 * i + 1] = i % 3 ? (1 << 28) : -(1 << 28);
    }
    int64_t Dx, Dy;
    for (uint32_t Y = 0; Y < 64; Y++)
        for (uint32_t X = 0; X < 257; X++) {
            CHECK(debig_png_elastic_displacement(g, 33, 33, 257, 64, X, Y, &Dx, &Dy) == 1);
            CHECK(Dx > -((int64_t)1 << 29) && Dx < ((int64_t)1 << 29) && Dy > -((int64_t)1 << 29) && Dy < ((int64_t)1 << 29));
        }
    for (uint32_t c = 0; c < 4; c++)
        CHECK(debig_png_elastic_displacement(g, 33, 33, 16384, 16384, c & 1 ? 16383 : 0, c & 2 ? 16383 : 0, &Dx, &Dy) == 1);
    CHECK(debig_png_elastic_displacement(g, 33, 33, 1, 1, 0, 0, &Dx, &Dy) == 1 && Dx == g[2 * (16 * 33 + 16)] && Dy == g[2 * (16 * 33 + 16) + 1]);
    int32_t *g2 = (int32_t *)malloc(2u * 2u * 2u * sizeof(int32_t));
    for (uint32_t i = 0; i < 8; i++) g2[i] = (int32_t)i * 65536;
    CHECK(debig_png_elastic_displacement(g2, 2, 2, 7, 3, 6, 2, &Dx, &Dy) == 1);
    CHECK(debig_png_elastic_displacement(g2, 1, 2, 7, 3, 0, 0, &Dx, &Dy) == 0 && debig_png_elastic_displacement(g2, 2, 34, 7, 3, 0, 0, &Dx, &Dy) == 0);
    CHECK(debig_png_elastic_displacement(g2, 2, 2, 7, 3, 7, 0, &Dx, &Dy) == 0 && debig_png_elastic_displacement(g2, 2, 2, 7, 3, 0, 3, &Dx, &Dy) == 0);
    CHECK(debig_png_elastic_displacement(g2, 2, 2, 0, 3, 0, 0, &Dx, &Dy) == 0 && debig_png_elastic_displacement(g2, 2, 2, 16385, 3, 0, 0, &Dx, &Dy) == 0);
    CHECK(debig_png_elastic_displacement(NULL, 2, 2, 7, 3, 0, 0, &Dx, &Dy) == 0);
    g2[7] = (1 << 28) + 1;
    CHECK(debig_png_elastic_displacement(g2, 2, 2, 7, 3, 0, 0, &Dx, &Dy) == 0);
    g2[7] = INT32_MIN;
    CHECK(debig_png_elastic_displacement(g2, 2, 2, 7, 3, 0, 0, &Dx, &Dy) == 0);
    free(g);
    free(g2);

    /* ---- the calls.  Heap copies of exactly the files' and the fields' sizes */
    uint8_t tmp[64];
    const struct { uint32_t w, h; uint8_t depth, ct; } spec[N] = {{9, 7, 16, 2}, {9, 7, 8, 2}, {9, 7, 8, 3}, {9, 7, 4, 0}, {9, 7, 8, 0}};
    double *fields[N];
    for (uint32_t i = 0; i < N; i++) {
        sizes[i] = stub_png(tmp, spec[i].w, spec[i].h, spec[i].depth, spec[i].ct);
        files[i] = (uint8_t *)malloc(sizes[i]);
        memcpy(files[i], tmp, sizes[i]);
        const double id[6] = {1, 0, 0, 0, 1, 0};
        memcpy(warps[i].m, id, sizeof id);
        fields[i] = (double *)malloc(GW * GH * 2u * sizeof(double));
        for (uint32_t j = 0; j < GW * GH * 2u; j++) fields[i][j] = ((double)j - 14.5) / 4.0;
        elastics[i].nodes = fields[i];
    }
    const uint8_t *const *in = (const uint8_t *const *)files;
    debig_png_elastic_desc ed = {GW, GH, {0, 0}};

    debig_png_tensor_desc td;
    memset(&td, 0, sizeof td);
    td.out_w = 8; td.out_h = 6; td.out_format = DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8; td.dtype = DEBIG_PNG_T_F32;
    for (uint32_t j = 0; j < 4; j++) td.scale[j] = 1.0f;
    debig_png_warp_desc wd;
    memset(&wd, 0, sizeof wd);
    debig_png_color colors[N];
    debig_png_tone tones[N];
    debig_png_blur blurs[N];
    memset(colors, 0, sizeof colors);
    memset(tones, 0, sizeof tones);
    memset(blurs, 0, sizeof blurs);

    /* the tensor call's argument checks, through each of the four affine calls it stands for, then its own */
    for (uint32_t s = 0; s < 5; s++) { /* (and the blur call with blurs alone) */
        const debig_png_color *cs = s == 1 || s == 3 ? colors : NULL;
        const debig_png_tone *ts = s == 2 || s == 3 ? tones : NULL;
        const debig_png_blur *bs = s >= 3 ? blurs : NULL;
#define TENSOR(W_, TD_, WD_, ES_, ED_) debig_png_decode_batch_tensor_elastic(in, sizes, OUT, NULL, W_, cs, ts, NULL, 0, bs, status, NULL, N, 0, TD_, WD_, ES_, ED_)
        reset(); untouched(TENSOR(NULL, &td, &wd, elastics, &ed));
        reset(); untouched(TENSOR(warps, &td, NULL, elastics, &ed));
        reset(); untouched(TENSOR(NULL, &td, NULL, elastics, &ed));
        reset(); untouched(TENSOR(warps, NULL, &wd, elastics, &ed));
        wd.filter = DEBIG_PNG_FILTER_BICUBIC;
        reset(); untouched(TENSOR(warps, &td, &wd, elastics, &ed));
        wd.filter = DEBIG_PNG_FILTER_BILINEAR; wd.border_mode = 2;
        reset(); untouched(TENSOR(warps, &td, &wd, elastics, &ed));
        wd.border_mode = DEBIG_PNG_BORDER_CONSTANT; wd.alpha_mode = 1;
        reset(); untouched(TENSOR(warps, &td, &wd, elastics, &ed));
        wd.alpha_mode = 0;
        reset(); untouched(TENSOR(warps, &td, &wd, NULL, &ed));
        reset(); untouched(TENSOR(warps, &td, &wd, elastics, NULL));
        const debig_png_elastic_desc bad_ed[6] = {{1, 3, {0, 0}}, {5, 1, {0, 0}}, {34, 3, {0, 0}}, {5, 34, {0, 0}}, {5, 3, {1, 0}}, {5, 3, {0, 1}}};
        for (uint32_t b = 0; b < 6; b++) {
            reset(); untouched(TENSOR(warps, &td, &wd, elastics, &bad_ed[b]));
        }
    }
    CHECK(debig_png_decode_batch_tensor_elastic(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL) == 0);

    /* the statuses decided at IHDR: a bad box ahead of a bad field; NaN, a node of 4097, a bad matrix under a good field -- each
     * ahead of the missing IDAT; a good field, and no field, leave what the file lacks */
    const debig_png_box boxes[N] = {{0, 0, 10, 1}, {0, 0, 0, 0}, {1, 1, 8, 6}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    fields[0][3] = NAN;
    fields[1][GW * GH * 2u - 1u] = NAN;   /* the last double of the field */
    fields[2][0] = -4097.0;
    warps[3].m[1] = 32768.5;
    for (uint32_t s = 0; s < 3; s++) {
        elastics[4].nodes = s == 1 ? NULL : fields[4];
        reset();
        CHECK(debig_png_decode_batch_tensor_elastic(in, sizes, OUT, boxes, warps, s == 1 ? colors : NULL, s == 2 ? tones : NULL, NULL, 0,
                                                    s == 2 ? blurs : NULL, status, NULL, N, 0, &td, &wd, elastics, &ed) == 0);
        CHECK(status[0] == DEBIG_PNG_E_BOX && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
        CHECK(status[4] != 0 && status[4] != SENTINEL && status[4] != DEBIG_PNG_E_WARP);
    }

    debig_png_label_desc ld;
    memset(&ld, 0, sizeof ld);
    ld.out_w = 8; ld.out_h = 6; ld.dtype = DEBIG_PNG_L_I32;
    debig_png_label_warp_desc lw = {DEBIG_PNG_BORDER_CONSTANT, -1};
    reset(); untouched(debig_png_decode_batch_labels_elastic(in, sizes, OUT, NULL, NULL, status, NULL, N, 0, &ld, &lw, elastics, &ed));
    reset(); untouched(debig_png_decode_batch_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, N, 0, &ld, NULL, elastics, &ed));
    reset(); untouched(debig_png_decode_batch_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, N, 0, &ld, &lw, NULL, &ed));
    reset(); untouched(debig_png_decode_batch_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, N, 0, &ld, &lw, elastics, NULL));
    ed.grid_w = 34;
    reset(); untouched(debig_png_decode_batch_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, N, 0, &ld, &lw, elastics, &ed));
    ed.grid_w = GW;
    lw.border_mode = 2;
    reset(); untouched(debig_png_decode_batch_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, N, 0, &ld, &lw, elastics, &ed));
    lw.border_mode = DEBIG_PNG_BORDER_CONSTANT;
    reset();
    CHECK(debig_png_decode_batch_labels_elastic(in, sizes, OUT, boxes, warps, status, NULL, N, 0, &ld, &lw, elastics, &ed) == 0);
    CHECK(status[0] == DEBIG_PNG_E_LABEL && status[1] == DEBIG_PNG_E_LABEL && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
    CHECK(status[4] != 0 && status[4] != SENTINEL && status[4] != DEBIG_PNG_E_WARP);
    CHECK(debig_png_decode_batch_labels_elastic(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL) == 0);

    uint32_t keys[3] = {1, 2, 3};
    int32_t values[3] = {4, 5, 6};
    debig_png_color_map map = {3, 0, keys, values};
    debig_png_color_label_desc cd = {8, 6, DEBIG_PNG_L_I32, DEBIG_PNG_CL_MAP, -1, 1, &map, 0, 0};
    reset(); untouched(debig_png_decode_batch_color_labels_elastic(in, sizes, OUT, NULL, NULL, status, NULL, unmatched, N, 0, &cd, &lw, elastics, &ed));
    reset(); untouched(debig_png_decode_batch_color_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, unmatched, N, 0, &cd, NULL, elastics, &ed));
    reset(); untouched(debig_png_decode_batch_color_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, unmatched, N, 0, &cd, &lw, NULL, &ed));
    ed.reserved[1] = 7; /* found after a table has been made */
    reset(); untouched(debig_png_decode_batch_color_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, unmatched, N, 0, &cd, &lw, elastics, &ed));
    ed.reserved[1] = 0;
    cd.n_maps = 2; /* an inherited check */
    reset(); untouched(debig_png_decode_batch_color_labels_elastic(in, sizes, OUT, NULL, warps, status, NULL, unmatched, N, 0, &cd, &lw, elastics, &ed));
    cd.n_maps = 1;
    reset();
    CHECK(debig_png_decode_batch_color_labels_elastic(in, sizes, OUT, boxes, warps, status, NULL, unmatched, N, 0, &cd, &lw, elastics, &ed) == 0);
    CHECK(status[0] == DEBIG_PNG_E_LABEL && status[1] == DEBIG_PNG_E_WARP && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
    CHECK(status[4] != 0 && status[4] != SENTINEL && status[4] != DEBIG_PNG_E_WARP);
    for (uint32_t i = 0; i < N; i++) CHECK(unmatched[i] == 0);
    CHECK(debig_png_decode_batch_color_labels_elastic(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL) == 0);

    for (uint32_t i = 0; i < N; i++) {
        free(files[i]);
        free(fields[i]);
    }
    puts("asan_png_elastic: all checks passed");
    return 0;
}
