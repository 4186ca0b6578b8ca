/* DEVELOPMENT / TEST TOOLING: the four kernels of the perspective warp (csrc/png_persp_kernel.inc) on the CPU lock-step emulator
 * under AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_persp_emu.sh links it with the emulator sources compiled
 * under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * Every buffer is a heap block of exactly its size, so a tap outside the arena or a store outside the tensor is ASan's to see, and
 * a shift or a division outside its range is UBSan's.  Each kernel runs a few tasks -- a keystone, D from 2^21 up to just below 2^33
 * along a row, positions about 2^51 and, on the last row of a 16384 x 16384 output, about 2^58, a map that leaves the crop on the
 * negative side -- under both borders, NEAREST compared with a restatement in 128-bit integers, BILINEAR run for the sanitizers (the
 * pytest battery compares it bit for bit); then the tasks that break a bound, which must leave the sentinels as they are. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/debig_hip.h"

extern "C" int emu_png_persp_batch(const void *, void *, const debig_png_persp_task *, uint32_t, uint32_t);
extern "C" int emu_png_persp_color_batch(const void *, void *, const debig_png_persp_color_task *, const void *, uint32_t, uint32_t);
extern "C" int emu_png_label_persp_batch(const void *, void *, const debig_png_label_persp_task *, const int32_t *, uint32_t, uint32_t);
extern "C" int emu_png_color_label_persp_batch(const void *, void *, const debig_png_color_label_persp_task *, const void *, uint32_t *,
                                               uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define FILL 0xEE

enum { SW = 17, SH = 12, BX = 3, BY = 4, CW = 13, CH = 7, W = 20, H = 6 }; /* the image, the crop inside it, the output */

struct Map { int64_t m[6], p[3]; };
static const int64_t D_MIN = (int64_t)1 << 21, D_MAX = ((int64_t)1 << 33) - 1;

/* the pick of output pixel (X, Y): floor(N 2^31 / D) >> 17 in 128-bit integers */
static void pick(const Map &a, uint32_t X, uint32_t Y, int64_t *jx, int64_t *jy)
{
    const int64_t cx = 2 * (int64_t)X + 1, cy = 2 * (int64_t)Y + 1;
    const __int128 D = a.p[0] * cx + a.p[1] * cy + 2 * a.p[2];
    const __int128 n[2] = {a.m[0] * cx + a.m[1] * cy + 2 * a.m[2], a.m[3] * cx + a.m[4] * cy + 2 * a.m[5]};
    int64_t j[2];
    for (int k = 0; k < 2; k++) {
        const __int128 num = n[k] * ((__int128)1 << 31);
        __int128 q = num / D;
        if (num % D != 0 && num < 0) q--;
        j[k] = (int64_t)(q >> 17);
    }
    *jx = j[0];
    *jy = j[1];
}

static bool inside(int64_t jx, int64_t jy) { return jx >= 0 && jx < CW && jy >= 0 && jy < CH; }
static uint32_t clampi(int64_t j, int64_t n) { return (uint32_t)(j < 0 ? 0 : j >= n ? n - 1 : j); }

template <class T> static T *heap(size_t n, int fill)
{
    T *p = (T *)malloc(n * sizeof(T));
    CHECK(p);
    memset(p, fill, n * sizeof(T));
    return p;
}

static bool all_fill(const uint8_t *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (p[i] != FILL) return false;
    return true;
}

template <class Task> static void put_map(Task &t, const Map &a)
{
    memcpy(t.m, a.m, sizeof a.m);
    memcpy(t.p, a.p, sizeof a.p);
}

/* the p[] that break a bound on the W x H output (with the identity in rows 0 and 1) */
static const int64_t BAD_P[][3] = {
    {((int64_t)1 << 32) + 1, 0, -((int64_t)1 << 32)}, {0, -((int64_t)1 << 32) - 1, (int64_t)1 << 32}, {0, 0, ((int64_t)1 << 32) + 1},
    {0, 0, 0}, {0, 0, -((int64_t)1 << 30)}, {0, 0, ((int64_t)1 << 20) - 1}, {1, 0, ((int64_t)1 << 20) - 1},
    {1, 0, ((int64_t)1 << 32) + 1 - W}, {-((int64_t)1 << 26), 0, (int64_t)1 << 30}, {0, -((int64_t)1 << 28), (int64_t)1 << 30},
    {(int64_t)1 << 27, (int64_t)1 << 29, (int64_t)1 << 30}};
enum { N_BAD = sizeof BAD_P / sizeof BAD_P[0] };

int main()
{
    /* the maps */
    const int64_t slope = ((D_MAX - D_MIN) / (2 * (W - 1))) & ~(int64_t)1;
    const Map maps[] = {
        {{40000, 3000, -70000, -2000, 50000, 30000}, {3 << 18, -(1 << 18), 1 << 30}},                            /* a keystone        */
        {{4 * 65536 * CW / W, 0, 0, 0, 4 * 65536 * CH / H, 0}, {slope, 0, (D_MIN - slope) / 2}},                  /* D from 2^21       */
        {{65536, 0, (int64_t)1 << 40, 0, 65536, -((int64_t)1 << 40)}, {0, 0, 1 << 20}},                           /* |U| about 2^51    */
        {{81920, 6554, -655360, 3277, 58982, -288358}, {2147483, 1073741, 1 << 30}},                              /* the negative side */
        {{65536, 0, 0, 0, 65536, 0}, {0, 0, 1 << 30}}};                                                           /* the identity      */
    const uint32_t n_maps = sizeof maps / sizeof maps[0];
    for (uint32_t k = 0; k < n_maps; k++)
        for (uint32_t c = 0; c < 4; c++) {
            const int64_t D = maps[k].p[0] * (c & 1 ? 2 * W - 1 : 1) + maps[k].p[1] * (c & 2 ? 2 * H - 1 : 1) + 2 * maps[k].p[2];
            CHECK(D >= D_MIN && D <= D_MAX);
        }

    /* ---- the image kernel and the colour kernel (an identity record): RGB8, UINT, HWC */
    const size_t src_n = (size_t)SW * SH * 3;
    uint8_t *src = heap<uint8_t>(src_n, 0);
    for (size_t i = 0; i < src_n; i++) src[i] = (uint8_t)(i * 37u + 11u);
    const size_t slot = (size_t)H * W * 3;
    debig_png_color_rec *rec = heap<debig_png_color_rec>(1, 0);
    rec->k[0] = rec->k[4] = rec->k[8] = 65536;
    for (uint32_t border = 0; border < 2; border++)
        for (uint32_t filter = 0; filter < 3; filter += 2)
            for (uint32_t color = 0; color < 2; color++) {
                const uint32_t rows = 4, per = (H + rows - 1) / rows, n = n_maps * per;
                debig_png_persp_color_task *ct = heap<debig_png_persp_color_task>(n, 0);
                debig_png_persp_task *pt = heap<debig_png_persp_task>(n, 0);
                for (uint32_t k = 0; k < n_maps; k++)
                    for (uint32_t r = 0; r < per; r++) {
                        debig_png_persp_color_task &t = ct[k * per + r];
                        t.src_off = ((size_t)BY * SW + BX) * 3; t.out_off = k * slot; t.src_pitch = SW * 3; t.crop_w = CW; t.crop_h = CH;
                        t.out_w = W; t.out_h = H; t.row0 = r * rows; t.rows = H - r * rows < rows ? H - r * rows : rows;
                        t.out_sx = 3; t.out_sy = 3 * W; t.out_sc = 1; t.channels = 3; t.bits = 8; t.dtype = 0; t.filter = (uint8_t)filter;
                        t.border_mode = (uint8_t)border; t.border[0] = 201; t.border[1] = 202; t.border[2] = 203;
                        put_map(t, maps[k]);
                        memcpy(&pt[k * per + r], &t, offsetof(debig_png_persp_task, p)); /* field for field up to p[] */
                        put_map(pt[k * per + r], maps[k]);
                    }
                uint8_t *out = heap<uint8_t>(n_maps * slot, FILL);
                CHECK((color ? emu_png_persp_color_batch(src, out, ct, rec, n, 2) : emu_png_persp_batch(src, out, pt, n, 2)) == 0);
                for (uint32_t k = 0; k < n_maps && filter == 2; k++)
                    for (uint32_t Y = 0; Y < H; Y++)
                        for (uint32_t X = 0; X < W; X++) {
                            int64_t jx, jy;
                            pick(maps[k], X, Y, &jx, &jy);
                            for (uint32_t c = 0; c < 3; c++) {
                                const uint8_t want = border || inside(jx, jy) ? src[((BY + clampi(jy, CH)) * SW + BX + clampi(jx, CW)) * 3 + c]
                                                                              : (uint8_t)(201 + c);
                                CHECK(out[k * slot + (Y * W + X) * 3 + c] == want);
                            }
                        }
                free(out);
                free(ct);
                free(pt);
            }
    /* numerators near 2^48 over D = 2^21: the last row of a 16384 x 16384 output as one task whose out_sy is 0 */
    {
        debig_png_persp_task *t = heap<debig_png_persp_task>(1, 0);
        const Map far = {{(int64_t)1 << 31, (int64_t)1 << 31, (int64_t)1 << 40, -((int64_t)1 << 31), -((int64_t)1 << 31), -((int64_t)1 << 40)},
                         {0, 0, 1 << 20}};
        t->src_off = ((size_t)BY * SW + BX) * 3; t->src_pitch = SW * 3; t->crop_w = CW; t->crop_h = CH; t->out_w = t->out_h = 16384;
        t->row0 = 16383; t->rows = 1; t->out_sx = 3; t->out_sy = 0; t->out_sc = 1; t->channels = 3; t->bits = 8; t->border_mode = 1;
        put_map(*t, far);
        uint8_t *out = heap<uint8_t>(16384 * 3, FILL);
        for (uint32_t filter = 0; filter < 3; filter += 2) {
            t->filter = (uint8_t)filter;
            CHECK(emu_png_persp_batch(src, out, t, 1, 0) == 0);
            for (uint32_t i = 0; i < 16384 * 3; i++) CHECK(out[i] == src[(BY * SW + BX + CW - 1) * 3 + i % 3]); /* the top right pixel */
        }
        free(out);
        free(t);
    }
    /* tasks that break a bound */
    {
        const uint32_t n = N_BAD + 2;
        debig_png_persp_task *pt = heap<debig_png_persp_task>(n, 0);
        debig_png_persp_color_task *ct = heap<debig_png_persp_color_task>(n, 0);
        for (uint32_t k = 0; k < n; k++) {
            debig_png_persp_color_task &t = ct[k];
            t.src_pitch = SW * 3; t.crop_w = SW; t.crop_h = SH; t.out_w = W; t.out_h = H; t.rows = k & 1 ? 1 : H; t.out_sx = 3; t.out_sy = 3 * W;
            t.out_sc = 1; t.channels = 3; t.bits = 8;
            t.m[0] = t.m[4] = 65536;
            if (k < N_BAD) memcpy(t.p, BAD_P[k], sizeof t.p);
            else { t.p[2] = 1 << 30; if (k == N_BAD) t.m[0] = ((int64_t)1 << 31) + 1; else t.out_w = 16385; }
            memcpy(&pt[k], &t, offsetof(debig_png_persp_task, p));
            memcpy(pt[k].p, t.p, sizeof t.p);
        }
        uint8_t *out = heap<uint8_t>(slot, FILL);
        CHECK(emu_png_persp_batch(src, out, pt, n, 3) == 0 && all_fill(out, slot));
        CHECK(emu_png_persp_color_batch(src, out, ct, rec, n, 0) == 0 && all_fill(out, slot));
        free(out);
        free(pt);
        free(ct);
    }
    free(rec);
    free(src);

    /* ---- the label kernel: 16-bit labels into int64, and bytes through a LUT into uint16 */
    {
        uint16_t *lab = heap<uint16_t>((size_t)SW * SH, 0);
        uint8_t *lab8 = heap<uint8_t>((size_t)SW * SH, 0);
        for (uint32_t i = 0; i < SW * SH; i++) { lab[i] = (uint16_t)(i * 251u + 7u); lab8[i] = (uint8_t)(i * 13u + 5u); }
        int32_t *lut = heap<int32_t>(256, 0);
        for (uint32_t i = 0; i < 256; i++) lut[i] = (int32_t)(i * 257u);
        for (uint32_t wide = 0; wide < 2; wide++)
            for (uint32_t border = 0; border < 2; border++) {
                const uint32_t n = n_maps * 3, es = wide ? 8u : 2u;
                debig_png_label_persp_task *lt = heap<debig_png_label_persp_task>(n, 0);
                for (uint32_t k = 0; k < n_maps; k++)
                    for (uint32_t r = 0; r < 3; r++) {
                        debig_png_label_persp_task &t = lt[k * 3 + r];
                        t.src_bytes = wide ? 2 : 1; t.src_off = ((size_t)BY * SW + BX) * t.src_bytes; t.out_off = (size_t)k * H * W * es;
                        t.src_pitch = SW; t.crop_w = CW; t.crop_h = CH; t.out_w = W; t.out_h = H; t.row0 = 2 * r; t.rows = 2; t.border_label = 999;
                        t.dtype = wide ? 3 : 1; t.border_mode = (uint8_t)border;
                        put_map(t, maps[k]);
                    }
                uint8_t *out = heap<uint8_t>((size_t)n_maps * H * W * es, FILL);
                CHECK(emu_png_label_persp_batch(wide ? (const void *)lab : (const void *)lab8, out, lt, wide ? NULL : lut, n, 4) == 0);
                for (uint32_t k = 0; k < n_maps; k++)
                    for (uint32_t Y = 0; Y < H; Y++)
                        for (uint32_t X = 0; X < W; X++) {
                            int64_t jx, jy;
                            pick(maps[k], X, Y, &jx, &jy);
                            const size_t at = (BY + clampi(jy, CH)) * SW + BX + clampi(jx, CW), el = ((size_t)k * H + Y) * W + X;
                            const int64_t want = border || inside(jx, jy) ? (wide ? (int64_t)lab[at] : (int64_t)(uint16_t)lut[lab8[at]]) : 999;
                            int64_t got;
                            if (wide) memcpy(&got, out + el * 8, 8);
                            else { uint16_t g; memcpy(&g, out + el * 2, 2); got = g; }
                            CHECK(got == want);
                        }
                free(out);
                free(lt);
            }
        debig_png_label_persp_task *lt = heap<debig_png_label_persp_task>(N_BAD, 0);
        for (uint32_t k = 0; k < N_BAD; k++) {
            debig_png_label_persp_task &t = lt[k];
            t.src_bytes = 1; t.src_pitch = SW; t.crop_w = SW; t.crop_h = SH; t.out_w = W; t.out_h = H; t.rows = k & 1 ? 1 : H; t.dtype = 2;
            t.m[0] = t.m[4] = 65536;
            memcpy(t.p, BAD_P[k], sizeof t.p);
        }
        uint8_t *out = heap<uint8_t>((size_t)H * W * 4, FILL);
        CHECK(emu_png_label_persp_batch(lab8, out, lt, lut, N_BAD, 0) == 0 && all_fill(out, (size_t)H * W * 4));
        free(out);
        free(lt);
        free(lut);
        free(lab8);
        free(lab);
    }

    /* ---- the colour-label kernel: PACK into int32; MAP into uint8 through an empty table of two slots */
    {
        uint8_t *rgb = heap<uint8_t>((size_t)SW * SH * 3, 0); /* ends with the last pixel's last byte */
        for (uint32_t i = 0; i < SW * SH; i++) { rgb[3 * i] = (uint8_t)(i % 5u); rgb[3 * i + 1] = (uint8_t)(i % 3u); rgb[3 * i + 2] = 0; }
        uint32_t *table = heap<uint32_t>(4, 0xFF); /* two slots of (key, value), both empty */
        for (uint32_t border = 0; border < 2; border++)
            for (uint32_t mode = 0; mode < 2; mode++) {
                const uint32_t n = n_maps * 2, es = mode ? 1u : 4u;
                debig_png_color_label_persp_task *t0 = heap<debig_png_color_label_persp_task>(n, 0);
                for (uint32_t k = 0; k < n_maps; k++)
                    for (uint32_t r = 0; r < 2; r++) {
                        debig_png_color_label_persp_task &t = t0[k * 2 + r];
                        t.src_off = ((size_t)BY * SW + BX) * 3; t.out_off = (size_t)k * H * W * es; t.src_pitch = SW; t.crop_w = CW; t.crop_h = CH;
                        t.out_w = W; t.out_h = H; t.row0 = 3 * r; t.rows = 3; t.border_label = 77; t.dtype = mode ? 0 : 2; t.mode = (uint8_t)mode;
                        t.border_mode = (uint8_t)border; t.image = k; t.map_slots = 2; t.missing = 250;
                        put_map(t, maps[k]);
                    }
                uint8_t *out = heap<uint8_t>((size_t)n_maps * H * W * es, FILL);
                uint32_t *cnt = heap<uint32_t>(n_maps, 0);
                if (mode == 0) {
                    CHECK(emu_png_color_label_persp_batch(rgb, out, t0, table, NULL, n, 3) == 0);
                    for (uint32_t k = 0; k < n_maps; k++)
                        for (uint32_t Y = 0; Y < H; Y++)
                            for (uint32_t X = 0; X < W; X++) {
                                int64_t jx, jy;
                                pick(maps[k], X, Y, &jx, &jy);
                                const uint8_t *p = rgb + ((BY + clampi(jy, CH)) * SW + BX + clampi(jx, CW)) * 3;
                                const int32_t want = border || inside(jx, jy) ? (int32_t)(p[0] | p[1] << 8 | p[2] << 16) : 77;
                                int32_t got;
                                memcpy(&got, out + (((size_t)k * H + Y) * W + X) * 4, 4);
                                CHECK(got == want);
                            }
                } else {
                    /* an EMPTY table (every key 0xFFFFFFFF, which no colour packs to): every kept element is `missing` and counted */
                    CHECK(emu_png_color_label_persp_batch(rgb, out, t0, table, cnt, n, 3) == 0);
                    for (uint32_t k = 0; k < n_maps; k++) {
                        uint32_t kept = 0;
                        for (uint32_t Y = 0; Y < H; Y++)
                            for (uint32_t X = 0; X < W; X++) {
                                int64_t jx, jy;
                                pick(maps[k], X, Y, &jx, &jy);
                                const bool keep = border || inside(jx, jy);
                                kept += keep;
                                CHECK(out[((size_t)k * H + Y) * W + X] == (keep ? 250 : 77));
                            }
                        CHECK(cnt[k] == kept);
                    }
                }
                free(cnt);
                free(out);
                free(t0);
            }
        debig_png_color_label_persp_task *bt = heap<debig_png_color_label_persp_task>(N_BAD, 0);
        for (uint32_t k = 0; k < N_BAD; k++) {
            debig_png_color_label_persp_task &t = bt[k];
            t.src_pitch = SW; t.crop_w = SW; t.crop_h = SH; t.out_w = W; t.out_h = H; t.rows = k & 1 ? 1 : H; t.dtype = 2;
            t.m[0] = t.m[4] = 65536;
            memcpy(t.p, BAD_P[k], sizeof t.p);
        }
        uint8_t *out = heap<uint8_t>((size_t)H * W * 4, FILL);
        CHECK(emu_png_color_label_persp_batch(rgb, out, bt, table, NULL, N_BAD, 0) == 0 && all_fill(out, (size_t)H * W * 4));
        free(out);
        free(bt);
        free(table);
        free(rgb);
    }
    puts("asan_png_persp_emu: all checks passed");
    return 0;
}
