/* DEVELOPMENT / TEST TOOLING: the two label-distance kernels (csrc/png_label_distance_kernel.inc) on the CPU lock-step emulator
 * under AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_label_distance_emu.sh links it with the emulator sources
 * compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * The labels, the g planes and the output are heap blocks of exactly their sizes: every image starts one element behind a multiple
 * of 16 bytes and the block ends with the last element of the last image, so a load or a store in front of or behind any of them (the
 * row above a task's first row, the neighbour of a row's last element, a stack slot outside the column) is ASan's to see, and a
 * shift, a signed overflow in the envelope's arithmetic or an index outside its range is UBSan's.  The shapes are the extreme ones
 * of the pytest battery (tests/test_emu_png_label_distance.py) -- 1 x 1, 1 x 7, 9 x 1, widths around the segment and strip sizes,
 * columns that alternate every row, a lone site in a corner of 3 x 16384 and of 16384 x 3, a column of 16384 equal row distances
 * (the stack at its full depth), both modes, both formats, caps 0, 1 and 32767, cuts and grids -- compared with a brute-force
 * restatement of the rule in this file; then the tasks that break a bound, which must leave their outputs as they are. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"

extern "C" int emu_png_label_distance_rows_batch(const void *, void *, const debig_png_label_distance_rows_task *, uint32_t, uint32_t);
extern "C" int emu_png_label_distance_cols_batch(const void *, void *, const debig_png_label_distance_cols_task *, uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Image { uint32_t w, h, kind; uint64_t off, g_off, out_off; std::vector<int64_t> v; };

/* kind 0: blocks of ids with the ends of the dtype and values that differ in the high word only among them; 1: columns that
 * alternate every row; 2: one site in the last corner; 3: a first column of ones */
static int64_t value(const Image &im, uint32_t i, uint32_t x, uint32_t y, uint32_t dtype)
{
    static const int64_t lo[4] = {0, 0, INT32_MIN, INT64_MIN}, hi[4] = {255, 65535, INT32_MAX, INT64_MAX};
    if (im.kind == 1) return (x + y) % 2u + (x % 3u == 0 ? 1 : 0);
    if (im.kind == 2) return x + 1 == im.w && y + 1 == im.h ? 1 : 0;
    if (im.kind == 3) return x == 0 ? 1 : 0;
    const uint32_t b = (x / 6u + 5u * (y / 4u) + i) * 2654435761u >> 20;
    if (b % 17u == 0) return hi[dtype];
    if (b % 19u == 0) return lo[dtype];
    if (b % 23u == 0) return dtype == 3 ? ((int64_t)1 << 32) + 1 : 1;
    return (int64_t)(b % 3u);
}

static void put(uint8_t *p, uint32_t es, int64_t v) { memcpy(p, &v, es); } /* (little endian: the low bytes) */

static int64_t stored(int64_t v, uint32_t dtype)
{
    return dtype == 0 ? (int64_t)(uint8_t)v : dtype == 1 ? (int64_t)(uint16_t)v : dtype == 2 ? (int64_t)(int32_t)v : v;
}

/* the rule by brute force: -1 for NONE.  (The long images have few sites or a known answer: see below.) */
static int64_t d2_of(const Image &im, uint32_t x, uint32_t y, uint32_t sites, int64_t to)
{
    const int64_t v = im.v[(size_t)y * im.w + x];
    int64_t best = -1;
    for (uint32_t yy = 0; yy < im.h; yy++)
        for (uint32_t xx = 0; xx < im.w; xx++) {
            const int64_t u = im.v[(size_t)yy * im.w + xx];
            if (sites ? u != to : u == v) continue;
            const int64_t dx = (int64_t)x - xx, dy = (int64_t)y - yy, d = dx * dx + dy * dy;
            if (best < 0 || d < best) best = d;
        }
    return best;
}

static int64_t expected(const Image &im, uint32_t x, uint32_t y, uint32_t sites, int64_t to)
{
    if (im.kind == 2) { /* one site in the last corner: its own nearest site under DIFFERS is a neighbour */
        const int64_t dx = (int64_t)im.w - 1 - x, dy = (int64_t)im.h - 1 - y;
        const bool corner = dx == 0 && dy == 0;
        if (sites) return to == 1 ? dx * dx + dy * dy : to == 0 ? (corner ? 1 : 0) : -1;
        return corner ? 1 : dx * dx + dy * dy;
    }
    if (im.kind == 3) { /* a first column of ones, three columns */
        if (sites) return to == 1 ? (int64_t)x * x : to == 0 ? (x == 0 ? 1 : 0) : -1;
        return x == 2 ? 4 : 1;
    }
    return d2_of(im, x, y, sites, to);
}

int main()
{
    static const uint32_t shapes[][3] = {{1, 1, 0}, {7, 1, 0}, {1, 9, 0}, {63, 5, 0}, {64, 3, 0}, {65, 24, 0}, {33, 24, 0}, {70, 40, 0},
                                         {9, 17, 1}, {2, 5, 1}, {16384, 3, 2}, {3, 16384, 2}, {3, 16384, 3}};
    static const uint32_t caps[] = {0, 1, 32767, 5};
    uint32_t round = 0;
    for (uint32_t dtype = 0; dtype < 4; dtype++) {
        const uint32_t es = 1u << dtype;
        std::vector<Image> ims;
        uint64_t at = 0, gt = 0, ot = 0;
        for (const uint32_t *s : shapes)
            if (s[2] < 2 || dtype == 0) ims.push_back({s[0], s[1], s[2], 0, 0, 0, {}}); /* (the long images once: uint8) */
        for (Image &im : ims) {
            at += (16u - at % 16u) % 16u + es; /* one element behind a multiple of 16 */
            gt += (16u - gt % 16u) % 16u + 2u;
            ot += (16u - ot % 16u) % 16u + 4u;
            im.off = at;
            im.g_off = gt;
            im.out_off = ot;
            at += (uint64_t)im.w * im.h * es;
            gt += (uint64_t)im.w * im.h * 2u;
            ot += (uint64_t)im.w * im.h * 4u;
        }
        uint8_t *labels;
        CHECK(posix_memalign((void **)&labels, 16, at) == 0); /* ends with the last element */
        memset(labels, 0x5A, at);
        for (uint32_t i = 0; i < ims.size(); i++) {
            Image &im = ims[i];
            im.v.resize((size_t)im.w * im.h);
            for (uint32_t y = 0; y < im.h; y++)
                for (uint32_t x = 0; x < im.w; x++) {
                    const int64_t v = stored(value(im, i, x, y, dtype), dtype);
                    im.v[(size_t)y * im.w + x] = v;
                    put(labels + im.off + ((uint64_t)y * im.w + x) * es, es, v);
                }
        }
        static const int64_t tos[] = {1, 0, 2, -1};
        for (uint32_t sites = 0; sites < 2; sites++)
            for (uint32_t k = 0; k < (sites ? 4u : 2u); k++, round++) {
                const int64_t to = sites ? tos[k] : 0;
                const uint32_t cap = caps[round % 4u], format = round % 2u;
                const uint32_t strip = round % 3u == 0 ? DEBIG_PNG_LABEL_DISTANCE_COLS : round % 3u == 1 ? 16u : 5u;
                std::vector<debig_png_label_distance_rows_task> rt;
                std::vector<debig_png_label_distance_cols_task> ct;
                for (const Image &im : ims) {
                    uint32_t run = im.w >= DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS ? 1u : DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS / im.w;
                    if (round % 2u && im.h <= 40 && im.w <= 70) run = 3; /* the host's cut and runs of three rows in turn */
                    for (uint32_t y0 = 0; y0 < im.h; y0 += run) {
                        debig_png_label_distance_rows_task t;
                        memset(&t, 0, sizeof t);
                        t.label_off = im.off; t.g_off = im.g_off; t.value = to; t.w = im.w; t.h = im.h; t.row0 = y0;
                        t.rows = im.h - y0 < run ? im.h - y0 : run; t.dtype = dtype; t.sites = sites;
                        rt.push_back(t);
                    }
                    const uint32_t sw = im.w > 70 ? DEBIG_PNG_LABEL_DISTANCE_COLS : strip;
                    for (uint32_t x0 = 0; x0 < im.w; x0 += sw) {
                        debig_png_label_distance_cols_task t;
                        memset(&t, 0, sizeof t);
                        t.g_off = im.g_off; t.out_off = im.out_off; t.w = im.w; t.h = im.h; t.x0 = x0; t.cols = im.w - x0 < sw ? im.w - x0 : sw;
                        t.cap = cap; t.format = format;
                        ct.push_back(t);
                    }
                }
                /* (exactly the tasks, the g planes and the output: heap blocks of their own) */
                debig_png_label_distance_rows_task *rk = (debig_png_label_distance_rows_task *)malloc(rt.size() * sizeof rt[0]);
                debig_png_label_distance_cols_task *ck = (debig_png_label_distance_cols_task *)malloc(ct.size() * sizeof ct[0]);
                uint8_t *g, *out;
                CHECK(posix_memalign((void **)&g, 16, gt) == 0 && posix_memalign((void **)&out, 16, ot) == 0 && rk && ck);
                memset(g, 0xEE, gt);
                memset(out, 0xEE, ot);
                memcpy(rk, rt.data(), rt.size() * sizeof rt[0]);
                memcpy(ck, ct.data(), ct.size() * sizeof ct[0]);
                CHECK(emu_png_label_distance_rows_batch(labels, g, rk, (uint32_t)rt.size(), round % 4u) == 0);
                CHECK(emu_png_label_distance_cols_batch(g, out, ck, (uint32_t)ct.size(), round % 3u) == 0);
                for (const Image &im : ims)
                    for (uint32_t y = 0; y < im.h; y++)
                        for (uint32_t x = 0; x < im.w; x++) {
                            const int64_t d = expected(im, x, y, sites, to);
                            const int64_t c2 = (int64_t)cap * cap;
                            const int64_t r = d < 0 ? (cap ? c2 : INT32_MAX) : (cap && c2 < d ? c2 : d);
                            const uint8_t *p = out + im.out_off + ((uint64_t)y * im.w + x) * 4u;
                            if (format == 0) {
                                const int32_t exp = (int32_t)r;
                                CHECK(memcmp(p, &exp, 4) == 0);
                            } else {
                                const float exp = d < 0 && !cap ? INFINITY : (float)sqrt((double)r);
                                CHECK(memcmp(p, &exp, 4) == 0);
                            }
                        }
                free(out);
                free(g);
                free(rk);
                free(ck);
            }

        /* the tasks that break a bound, over the 33 x 24 image as one run of rows and one strip */
        const Image *gi = nullptr;
        for (const Image &im : ims)
            if (im.w == 33 && im.h == 24) gi = &im;
        CHECK(gi);
        debig_png_label_distance_rows_task rgood;
        memset(&rgood, 0, sizeof rgood);
        rgood.label_off = gi->off; rgood.g_off = gi->g_off; rgood.w = 33; rgood.h = 24; rgood.rows = 24; rgood.dtype = dtype;
        std::vector<debig_png_label_distance_rows_task> rbad(16, rgood);
        rbad[0].dtype = 4; rbad[1].dtype = 0xffffffffu; rbad[2].sites = 2; rbad[3].w = 0; rbad[4].w = 16385; rbad[5].h = 0; rbad[6].h = 16385;
        rbad[7].rows = 0; rbad[8].rows = 25; rbad[9].row0 = 1; rbad[10].row0 = 24; rbad[11].row0 = 0xffffffffu; rbad[12].rows = 0xffffffffu;
        rbad[13].g_off = gi->g_off + 1; rbad[14].label_off = gi->off + es / 2u;
        if (es == 1) rbad[14].w = 0; /* (a byte has no misaligned offset) */
        rbad[15].w = 1000; rbad[15].h = 1000; rbad[15].rows = 17; /* more than 16384 elements in more than one row */
        debig_png_label_distance_cols_task cgood;
        memset(&cgood, 0, sizeof cgood);
        cgood.g_off = gi->g_off; cgood.out_off = gi->out_off; cgood.w = 33; cgood.h = 24; cgood.cols = 33;
        std::vector<debig_png_label_distance_cols_task> cbad(16, cgood);
        cbad[0].format = 2; cbad[1].format = 0xffffffffu; cbad[2].cap = 32768; cbad[3].w = 0; cbad[4].w = 16385; cbad[5].h = 0; cbad[6].h = 16385;
        cbad[7].cols = 0; cbad[8].cols = 34; cbad[9].cols = 65; cbad[10].x0 = 1; cbad[11].x0 = 33; cbad[12].x0 = 0xffffffffu;
        cbad[13].cols = 0xffffffffu; cbad[14].g_off = gi->g_off + 1; cbad[15].out_off = gi->out_off + 2;
        for (uint32_t grid = 0; grid < 2; grid++) {
            debig_png_label_distance_rows_task *rk = (debig_png_label_distance_rows_task *)malloc(rbad.size() * sizeof rbad[0]);
            debig_png_label_distance_cols_task *ck = (debig_png_label_distance_cols_task *)malloc(cbad.size() * sizeof cbad[0]);
            uint8_t *g = (uint8_t *)malloc(gt), *out = (uint8_t *)malloc(ot);
            CHECK(rk && ck && g && out);
            memset(g, 0xEE, gt);
            memset(out, 0xEE, ot);
            memcpy(rk, rbad.data(), rbad.size() * sizeof rbad[0]);
            memcpy(ck, cbad.data(), cbad.size() * sizeof cbad[0]);
            CHECK(emu_png_label_distance_rows_batch(labels, g, rk, (uint32_t)rbad.size(), grid) == 0);
            CHECK(emu_png_label_distance_cols_batch(g, out, ck, (uint32_t)cbad.size(), grid) == 0);
            for (uint64_t b = 0; b < gt; b++) CHECK(g[b] == 0xEE);
            for (uint64_t b = 0; b < ot; b++) CHECK(out[b] == 0xEE);
            free(out);
            free(g);
            free(rk);
            free(ck);
        }
        free(labels);
    }
    puts("asan_png_label_distance_emu: all checks passed");
    return 0;
}
