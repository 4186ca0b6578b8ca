/* DEVELOPMENT / TEST TOOLING: the host side of debig_png_decode_batch_color_labels_warp under AddressSanitizer and UBSan, as a
 * stand-alone CPU program (tools/asan_color_labels_warp.sh builds and runs it; no GPU, no Python).
 *
 * It links the C host layer (csrc/host/ *.c) compiled with -fsanitize=address,undefined against stubs of the debig_hip_* entry
 * points that abort when they are called: everything driven here -- the argument checks, the tables made during them, and the
 * statuses decided when IHDR has been read (E_LABEL > E_BOX > E_WARP > what comes later in the file) -- is decided on the
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

#define N 4
static uint8_t *files[N];
static uint64_t sizes[N];
static uint32_t status[N], unmatched[N];
static debig_png_warp warps[N];

static int call(const debig_png_color_label_desc *d, const debig_png_label_warp_desc *wd, const debig_png_warp *ws, const debig_png_box *bx)
{
    for (uint32_t i = 0; i < N; i++) status[i] = unmatched[i] = SENTINEL;
    return debig_png_decode_batch_color_labels_warp((const uint8_t *const *)files, sizes, (void *)(uintptr_t)0x10000, bx, ws, status,
                                                    NULL, unmatched, N, 0, d, wd);
}

static void untouched(int rc)
{
    CHECK(rc == DEBIG_PNG_BAD_ARG);
    for (uint32_t i = 0; i < N; i++) CHECK(status[i] == SENTINEL && unmatched[i] == SENTINEL);
}

int main(void)
{
    /* heap copies of exactly the files' sizes: a read past their end is ASan's to see */
    uint8_t tmp[64];
    const struct { uint32_t w, h; uint8_t depth, ct; } spec[N] = {{9, 7, 16, 2}, {9, 7, 8, 2}, {9, 7, 8, 3}, {9, 7, 4, 0}};
    for (uint32_t i = 0; i < N; i++) {
        sizes[i] = stub_png(tmp, spec[i].w, spec[i].h, spec[i].depth, spec[i].ct);
        files[i] = (uint8_t *)malloc(sizes[i]);
        memcpy(files[i], tmp, sizes[i]);
        const double id[6] = {1, 0, 0, 0, 1, 0};
        memcpy(warps[i].m, id, sizeof id);
    }

    /* a map of DEBIG_PNG_CMAP_MAX keys (the largest table) and small ones, one per image */
    uint32_t *keys = (uint32_t *)malloc(DEBIG_PNG_CMAP_MAX * sizeof(uint32_t));
    int32_t *values = (int32_t *)malloc(DEBIG_PNG_CMAP_MAX * sizeof(int32_t));
    for (uint32_t k = 0; k < DEBIG_PNG_CMAP_MAX; k++) { keys[k] = k * 8191u & 0xFFFFFFu; values[k] = (int32_t)(k & 255u); }
    debig_png_color_map maps[N] = {{DEBIG_PNG_CMAP_MAX, 0, keys, values}, {3, 0, keys, values}, {0, 0, NULL, NULL}, {1, 0, keys + 5, values + 5}};
    debig_png_color_label_desc d = {8, 6, DEBIG_PNG_L_U8, DEBIG_PNG_CL_MAP, 255, N, maps, 0, 0};
    debig_png_label_warp_desc wd = {DEBIG_PNG_BORDER_CONSTANT, 255};

    /* the warp's own argument checks: status and unmatched stay unwritten */
    untouched(call(&d, &wd, NULL, NULL));
    untouched(call(&d, NULL, warps, NULL));
    wd.border_mode = 2;
    untouched(call(&d, &wd, warps, NULL));
    wd.border_mode = DEBIG_PNG_BORDER_CONSTANT;
    wd.border_label = 256;
    untouched(call(&d, &wd, warps, NULL));
    d.dtype = DEBIG_PNG_L_U16;
    wd.border_label = -1;
    untouched(call(&d, &wd, warps, NULL));
    /* the inherited checks still come first: equal keys in the last map, found after three tables have been made */
    d.dtype = DEBIG_PNG_L_U8;
    uint32_t twice[2] = {4, 4};
    maps[N - 1].n = 2;
    maps[N - 1].keys = twice;
    untouched(call(&d, NULL, NULL, NULL));
    maps[N - 1].n = 1;
    maps[N - 1].keys = keys + 5;
    d.n_maps = N - 1;
    untouched(call(&d, &wd, warps, NULL));
    d.n_maps = N;
    d.missing = 256;
    untouched(call(&d, &wd, warps, NULL));
    d.missing = 255;
    CHECK(debig_png_decode_batch_color_labels_warp(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, NULL, NULL) == 0);

    /* the statuses decided at IHDR, in their order; CLAMP does not read border_label */
    wd.border_mode = DEBIG_PNG_BORDER_CLAMP;
    wd.border_label = -77;
    const debig_png_box boxes[N] = {{0, 0, 10, 1}, {3, 3, 0, 2}, {1, 1, 8, 6}, {0, 0, 0, 0}};
    warps[0].m[2] = NAN;                /* 16-bit, a bad box and a bad matrix: E_LABEL */
    warps[1].m[1] = 32768.5;            /* a bad box and a bad matrix: E_BOX */
    warps[2].m[5] = -16777216.0 - 4.0;  /* a good box, a bad matrix: E_WARP, ahead of the missing IDAT */
    warps[3].m[0] = INFINITY;           /* no box, a bad matrix: E_WARP */
    CHECK(call(&d, &wd, warps, boxes) == 0);
    CHECK(status[0] == DEBIG_PNG_E_LABEL && status[1] == DEBIG_PNG_E_BOX && status[2] == DEBIG_PNG_E_WARP && status[3] == DEBIG_PNG_E_WARP);
    for (uint32_t i = 0; i < N; i++) CHECK(unmatched[i] == 0);
    /* good matrices: what the file lacks (IDAT) decides, still on the host */
    for (uint32_t i = 1; i < N; i++) { const double id[6] = {1, 0, 0, 0, 1, 0}; memcpy(warps[i].m, id, sizeof id); }
    CHECK(call(&d, &wd, warps, NULL) == 0);
    CHECK(status[0] == DEBIG_PNG_E_LABEL);
    for (uint32_t i = 1; i < N; i++) CHECK(status[i] != 0 && status[i] != SENTINEL && status[i] != DEBIG_PNG_E_WARP && unmatched[i] == 0);

    for (uint32_t i = 0; i < N; i++) free(files[i]);
    free(keys);
    free(values);
    puts("asan_color_labels_warp: ok");
    return 0;
}
