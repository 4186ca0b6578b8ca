/* DEVELOPMENT / TEST TOOLING: the four kernels of the elastic deformation (csrc/png_elastic_kernel.inc) on the CPU lock-step
 * emulator under AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_elastic_emu.sh links it with the emulator
 * sources compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing
 * preloaded).
 *
 * Every buffer is a heap block of exactly its size -- the fields one block whose last grid, the largest, ends where the block
 * ends --, so a node read past the fields, a tap outside the arena or a store outside the tensor is ASan's to see, and a shift or
 * a sum outside its range is UBSan's.  Each kernel runs a few tasks -- a smooth field, nodes
 * alternating between +2^28 and -2^28 under matrix entries at their limits, no field, grids of 2 x 2, 3 x 5 and 33 x 33 -- under both
 * borders, NEAREST compared with a restatement of the rule in this file, BILINEAR run for the sanitizers (the pytest battery compares
 * it bit for bit); then the tasks that break a bound, one workgroup per task and one workgroup for all, which must leave the
 * sentinels as they are. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/debig_hip.h"

extern "C" int emu_png_elastic_batch(const void *, void *, const debig_png_elastic_task *, const void *, uint32_t, uint32_t);
extern "C" int emu_png_elastic_color_batch(const void *, void *, const debig_png_elastic_color_task *, const void *, const void *, uint32_t,
                                           uint32_t);
extern "C" int emu_png_label_elastic_batch(const void *, void *, const debig_png_label_elastic_task *, const int32_t *, const void *,
                                           uint32_t, uint32_t);
extern "C" int emu_png_color_label_elastic_batch(const void *, void *, const debig_png_color_label_elastic_task *, const void *, uint32_t *,
                                                 const void *, uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define FILL 0xEE
#define LIMIT ((int32_t)1 << 28)
#define NO_FIELD (~(uint64_t)0)

enum { SW = 17, SH = 12, BX = 3, BY = 4, CW = 13, CH = 7, W = 20, H = 6 }; /* the image, the crop inside it, the output */

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

/* ---- the rule, restated: the weights, the displacement and the pick of output pixel (X, Y) */
static void weights(int64_t t, int64_t w[4])
{
    const int64_t t2 = t * t, t3 = t2 * t, one = 16384, r = (int64_t)1 << 28;
    const int64_t n[4] = {-t3 + 2 * t2 * one - t * r, 3 * t3 - 5 * t2 * one + 2 * ((int64_t)1 << 42), -3 * t3 + 4 * t2 * one + t * r,
                          t3 - t2 * one};
    for (int j = 0; j < 4; j++) w[j] = (n[j] + r) >> 29;
    const int a = t < 8192 ? 1 : 2;
    w[a] = 0;
    w[a] = one - (w[0] + w[1] + w[2] + w[3]);
}

static void axis(uint32_t X, uint32_t n, uint32_t g, int64_t *k, int64_t w[4])
{
    const int64_t num = (2 * (int64_t)X + 1) * (g - 1), den = 2 * (int64_t)n;
    *k = num / den;
    weights(((num - *k * den) * 16384 + n) / den, w);
}

struct Field { const int32_t *q; uint32_t gw, gh; }; /* q NULL: no field */

static void pick(const int64_t m[6], const Field &f, uint32_t X, uint32_t Y, int64_t *jx, int64_t *jy)
{
    int64_t D[2] = {0, 0};
    if (f.q) {
        int64_t kx, ky, wx[4], wy[4], S[2] = {0, 0};
        axis(X, W, f.gw, &kx, wx);
        axis(Y, H, f.gh, &ky, wy);
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                int64_t r = ky - 1 + i, c = kx - 1 + j;
                r = r < 0 ? 0 : r > (int64_t)f.gh - 1 ? f.gh - 1 : r;
                c = c < 0 ? 0 : c > (int64_t)f.gw - 1 ? f.gw - 1 : c;
                for (int a = 0; a < 2; a++) S[a] += wy[i] * wx[j] * f.q[2 * (r * f.gw + c) + a];
            }
        for (int a = 0; a < 2; a++) D[a] = (S[a] + ((int64_t)1 << 27)) >> 28;
    }
    const int64_t cx = 2 * (int64_t)X + 1, cy = 2 * (int64_t)Y + 1;
    *jx = (m[0] * cx + m[1] * cy + 2 * m[2] + ((m[0] * D[0] + m[1] * D[1] + 16384) >> 15)) >> 17;
    *jy = (m[3] * cx + m[4] * cy + 2 * m[5] + ((m[3] * D[0] + m[4] * D[1] + 16384) >> 15)) >> 17;
}

static bool inside(int64_t jx, int64_t jy) { return jx >= 0 && jx < CW && jy >= 0 && jy < CH; }
static uint32_t clampi(int64_t j, int64_t n) { return (uint32_t)(j < 0 ? 0 : j >= n ? n - 1 : j); }

template <class Task> static void put_field(Task &t, uint64_t off, uint32_t gw, uint32_t gh)
{
    t.field_off = off;
    t.grid_w = (uint16_t)gw;
    t.grid_h = (uint16_t)gh;
}

/* (field_off, grid_w, grid_h) that break a bound; the offsets name the block made in main */
struct BadField { uint64_t off; uint32_t gw, gh; };

int main()
{
    /* ---- the fields: one heap block, every field at a multiple of 8 bytes, the last one ending where the block ends */
    const uint32_t n_smooth = 3 * 5 * 2, n_two = 2 * 2 * 2, n_big = 33 * 33 * 2;
    const uint64_t o_smooth = 0, o_two = o_smooth + n_smooth * 4, o_bad_first = o_two + n_two * 4, o_bad_last = o_bad_first + n_smooth * 4,
                   o_big_bad = o_bad_last + n_smooth * 4, o_big = o_big_bad + n_big * 4, end = o_big + n_big * 4;
    uint8_t *fields = heap<uint8_t>(end, 0);
    int32_t *smooth = (int32_t *)(fields + o_smooth), *two = (int32_t *)(fields + o_two), *big = (int32_t *)(fields + o_big);
    for (uint32_t i = 0; i < n_smooth; i++) smooth[i] = (int32_t)((i * 2654435761u) >> 12) % (6 << 16) - (3 << 16); /* up to 3 pixels */
    for (uint32_t i = 0; i < n_two; i++) two[i] = i % 2 ? -(40 << 16) : (25 << 16);
    for (uint32_t i = 0; i < n_big; i++) big[i] = (i / 2 + i / 66) % 2 ? -LIMIT : LIMIT; /* a checkerboard of the limits */
    memcpy(fields + o_bad_first, smooth, n_smooth * 4);
    memcpy(fields + o_bad_last, smooth, n_smooth * 4);
    ((int32_t *)(fields + o_bad_first))[0] = LIMIT + 1;
    ((int32_t *)(fields + o_bad_last))[n_smooth - 1] = -LIMIT - 1;
    ((int32_t *)(fields + o_big_bad))[n_big - 1] = INT32_MIN; /* the last node a workgroup stages */

    struct Job { int64_t m[6]; uint64_t off; Field f; };
    const int64_t lin = (int64_t)1 << 31, tr = (int64_t)1 << 40;
    const Job jobs[] = {
        {{40000, 3000, -70000, -2000, 50000, 30000}, o_smooth, {smooth, 5, 3}},
        {{65536 * CW / W, 0, 0, 0, 65536 * CH / H, 0}, o_two, {two, 2, 2}},
        {{65536 * CW / W, 0, 0, 0, 65536 * CH / H, 0}, o_big, {big, 33, 33}},
        {{lin, -lin, tr, -lin, lin, -tr}, o_big, {big, 33, 33}},          /* every entry at its limit under nodes at theirs */
        {{40000, 3000, -70000, -2000, 50000, 30000}, NO_FIELD, {NULL, 5, 3}},
        {{65536, 0, 0, 0, 65536, 0}, o_smooth, {smooth, 5, 3}}};
    const uint32_t n_jobs = sizeof jobs / sizeof jobs[0];

    const BadField bad[] = {{o_smooth, 1, 3}, {o_smooth, 5, 1}, {o_smooth, 0, 0}, {o_smooth, 34, 3}, {o_smooth, 5, 34}, {o_smooth, 65535, 65535},
                            {o_smooth + 4, 5, 3}, {o_smooth + 1, 5, 3}, {o_bad_first, 5, 3}, {o_bad_last, 5, 3}, {o_bad_last, 5, 3},
                            {o_big_bad, 33, 33}, {NO_FIELD, 1, 3}, {NO_FIELD, 5, 34}, {NO_FIELD - 8, 34, 34}};
    const uint32_t n_bad = sizeof bad / sizeof bad[0];

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
                const uint32_t rows = 4, per = (H + rows - 1) / rows, n = n_jobs * per;
                debig_png_elastic_color_task *ct = heap<debig_png_elastic_color_task>(n, 0);
                debig_png_elastic_task *pt = heap<debig_png_elastic_task>(n, 0);
                for (uint32_t k = 0; k < n_jobs; k++)
                    for (uint32_t r = 0; r < per; r++) {
                        debig_png_elastic_color_task &t = ct[k * per + r];
                        t.src_off = ((size_t)BY * SW + BX) * 3; t.out_off = k * slot; t.src_pitch = SW * 3; t.crop_w = CW; t.crop_h = CH;
                        t.out_w = W; t.out_h = H; t.row0 = r * rows; t.rows = H - r * rows < rows ? H - r * rows : rows;
                        t.out_sx = 3; t.out_sy = 3 * W; t.out_sc = 1; t.channels = 3; t.bits = 8; t.dtype = 0; t.filter = (uint8_t)filter;
                        t.border_mode = (uint8_t)border; t.border[0] = 201; t.border[1] = 202; t.border[2] = 203;
                        memcpy(t.m, jobs[k].m, sizeof t.m);
                        put_field(t, jobs[k].off, jobs[k].f.gw, jobs[k].f.gh);
                        memcpy(&pt[k * per + r], &t, offsetof(debig_png_elastic_task, field_off)); /* field for field up to there */
                        put_field(pt[k * per + r], jobs[k].off, jobs[k].f.gw, jobs[k].f.gh);
                    }
                uint8_t *out = heap<uint8_t>(n_jobs * slot, FILL);
                /* (two workgroups: each takes every other task, so it changes its grid and comes back to one it held) */
                CHECK((color ? emu_png_elastic_color_batch(src, out, ct, rec, fields, n, 2) : emu_png_elastic_batch(src, out, pt, fields, n, 2)) == 0);
                for (uint32_t k = 0; k < n_jobs && filter == 2; k++)
                    for (uint32_t Y = 0; Y < H; Y++)
                        for (uint32_t X = 0; X < W; X++) {
                            int64_t jx, jy;
                            pick(jobs[k].m, jobs[k].f, X, Y, &jx, &jy);
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

    /* the tasks that break a bound: the sentinels stay */
    {
        const uint32_t n = n_bad + 3;
        debig_png_elastic_task *pt = heap<debig_png_elastic_task>(n, 0);
        debig_png_elastic_color_task *ct = heap<debig_png_elastic_color_task>(n, 0);
        for (uint32_t k = 0; k < n; k++) {
            debig_png_elastic_color_task &t = ct[k];
            t.src_off = 0; t.src_pitch = SW * 3; t.crop_w = SW; t.crop_h = SH; t.out_w = W; t.out_h = H; t.rows = H; t.out_sx = 3;
            t.out_sy = 3 * W; t.out_sc = 1; t.channels = 3; t.bits = 8; t.m[0] = t.m[4] = 65536;
            if (k < n_bad) put_field(t, bad[k].off, bad[k].gw, bad[k].gh);
            else put_field(t, o_smooth, 5, 3);
            if (k == n_bad) t.out_w = 16385;          /* a bound of the warp twin under a good field */
            if (k == n_bad + 1) t.m[0] = lin + 1;
            if (k == n_bad + 2) t.filter = 1;
            memcpy(&pt[k], &t, offsetof(debig_png_elastic_task, field_off));
            put_field(pt[k], t.field_off, t.grid_w, t.grid_h);
        }
        uint8_t *out = heap<uint8_t>(slot, FILL);
        for (uint32_t g = 0; g < 2; g++) {
            CHECK(emu_png_elastic_batch(src, out, pt, fields, n, g) == 0 && all_fill(out, slot));
            CHECK(emu_png_elastic_color_batch(src, out, ct, rec, fields, n, g) == 0 && all_fill(out, slot));
        }
        free(out);
        free(pt);
        free(ct);
    }

    /* ---- the label kernel (8-bit labels through a LUT into int32) and the colour-label kernel (PACK into int32, MAP into uint8) */
    {
        const size_t lab_n = (size_t)SW * SH;
        uint8_t *lab = heap<uint8_t>(lab_n, 0);
        for (size_t i = 0; i < lab_n; i++) lab[i] = (uint8_t)(i * 29u + 5u);
        int32_t *lut = heap<int32_t>(256, 0);
        for (int i = 0; i < 256; i++) lut[i] = 1000 - 3 * i;
        uint32_t *table = heap<uint32_t>(16 * 2, 0xFF); /* 16 slots of (key, value), all empty: every in-crop pick misses */
        for (uint32_t border = 0; border < 2; border++) {
            const uint32_t rows = 4, per = (H + rows - 1) / rows, n = n_jobs * per;
            debig_png_label_elastic_task *lt = heap<debig_png_label_elastic_task>(n, 0);
            debig_png_color_label_elastic_task *kt = heap<debig_png_color_label_elastic_task>(2 * n, 0);
            for (uint32_t k = 0; k < n_jobs; k++)
                for (uint32_t r = 0; r < per; r++) {
                    debig_png_label_elastic_task &t = lt[k * per + r];
                    t.src_off = (size_t)BY * SW + BX; t.out_off = k * (size_t)H * W * 4; t.src_pitch = SW; t.crop_w = CW; t.crop_h = CH;
                    t.out_w = W; t.out_h = H; t.row0 = r * rows; t.rows = H - r * rows < rows ? H - r * rows : rows;
                    t.border_label = -7; t.src_bytes = 1; t.dtype = 2; t.border_mode = (uint8_t)border;
                    memcpy(t.m, jobs[k].m, sizeof t.m);
                    put_field(t, jobs[k].off, jobs[k].f.gw, jobs[k].f.gh);
                    for (uint32_t mode = 0; mode < 2; mode++) {
                        debig_png_color_label_elastic_task &c = kt[mode * n + k * per + r];
                        c.src_off = ((size_t)BY * SW + BX) * 3; c.out_off = mode ? n_jobs * (size_t)H * W * 4 + k * (size_t)H * W : k * (size_t)H * W * 4;
                        c.src_pitch = SW; c.crop_w = CW; c.crop_h = CH; c.out_w = W; c.out_h = H; c.row0 = t.row0; c.rows = t.rows;
                        c.border_label = mode ? 9 : -7; c.dtype = mode ? 0 : 2; c.mode = (uint8_t)mode; c.border_mode = (uint8_t)border;
                        c.map_slots = mode ? 16 : 0; c.missing = 250; c.image = k;
                        memcpy(c.m, jobs[k].m, sizeof c.m);
                        put_field(c, jobs[k].off, jobs[k].f.gw, jobs[k].f.gh);
                    }
                }
            int32_t *out = heap<int32_t>(n_jobs * (size_t)H * W, FILL);
            CHECK(emu_png_label_elastic_batch(lab, out, lt, lut, fields, n, 3) == 0);
            const size_t cl_bytes = n_jobs * (size_t)H * W * 5;
            uint8_t *cout = heap<uint8_t>(cl_bytes, FILL);
            uint32_t *um = heap<uint32_t>(n_jobs, 0);
            CHECK(emu_png_color_label_elastic_batch(src, cout, kt, table, um, fields, 2 * n, 3) == 0);
            for (uint32_t k = 0; k < n_jobs; k++) {
                uint32_t in_crop = 0;
                for (uint32_t Y = 0; Y < H; Y++)
                    for (uint32_t X = 0; X < W; X++) {
                        int64_t jx, jy;
                        pick(jobs[k].m, jobs[k].f, X, Y, &jx, &jy);
                        const bool keep = border || inside(jx, jy);
                        const size_t at = (BY + clampi(jy, CH)) * SW + BX + clampi(jx, CW);
                        CHECK(out[(k * H + Y) * W + X] == (keep ? lut[lab[at]] : -7));
                        const int32_t key = src[at * 3] | src[at * 3 + 1] << 8 | src[at * 3 + 2] << 16;
                        CHECK(((int32_t *)cout)[(k * H + Y) * W + X] == (keep ? key : -7));
                        CHECK(cout[n_jobs * (size_t)H * W * 4 + (k * H + Y) * W + X] == (keep ? 250 : 9));
                        in_crop += keep;
                    }
                CHECK(um[k] == in_crop);
            }
            free(out);
            free(cout);
            free(um);
            free(lt);
            free(kt);
        }
        /* the tasks that break a bound */
        debig_png_label_elastic_task *lt = heap<debig_png_label_elastic_task>(n_bad, 0);
        debig_png_color_label_elastic_task *kt = heap<debig_png_color_label_elastic_task>(n_bad, 0);
        for (uint32_t k = 0; k < n_bad; k++) {
            lt[k].src_pitch = SW; lt[k].crop_w = SW; lt[k].crop_h = SH; lt[k].out_w = W; lt[k].out_h = H; lt[k].rows = H; lt[k].src_bytes = 1;
            lt[k].dtype = 2; lt[k].m[0] = lt[k].m[4] = 65536;
            put_field(lt[k], bad[k].off, bad[k].gw, bad[k].gh);
            kt[k].src_pitch = SW; kt[k].crop_w = SW; kt[k].crop_h = SH; kt[k].out_w = W; kt[k].out_h = H; kt[k].rows = H; kt[k].dtype = 2;
            kt[k].m[0] = kt[k].m[4] = 65536;
            put_field(kt[k], bad[k].off, bad[k].gw, bad[k].gh);
        }
        uint8_t *out = heap<uint8_t>((size_t)H * W * 4, FILL);
        uint32_t *um = heap<uint32_t>(1, 0);
        for (uint32_t g = 0; g < 2; g++) {
            CHECK(emu_png_label_elastic_batch(lab, out, lt, NULL, fields, n_bad, g) == 0 && all_fill(out, (size_t)H * W * 4));
            CHECK(emu_png_color_label_elastic_batch(src, out, kt, table, um, fields, n_bad, g) == 0 && all_fill(out, (size_t)H * W * 4) && um[0] == 0);
        }
        free(out);
        free(um);
        free(lt);
        free(kt);
        free(lab);
        free(lut);
        free(table);
    }

    free(src);
    free(rec);
    free(fields);
    puts("asan_png_elastic_emu: all checks passed");
    return 0;
}
