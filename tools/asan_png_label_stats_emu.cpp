/* DEVELOPMENT / TEST TOOLING: the label-statistics kernel (csrc/png_label_stats_kernel.inc) on the CPU lock-step emulator under
 * AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_label_stats_emu.sh links it with the emulator sources
 * compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * Every buffer is a heap block of exactly its size: the label block ends with the last element of the last image and starts every
 * image one element behind a multiple of 16 bytes, the record block holds the records and nothing else, so a load in front of or
 * behind the labels (the 16-byte items end exactly where the run ends, or the tail is read element by element) or a record past
 * n_ids is ASan's to see, and a shift or an index outside its range is UBSan's.  The shapes are the extreme ones of the pytest
 * battery (tests/test_emu_png_label_stats.py) -- 1 x 1, widths 1, 7, 9, 33 and 70, heights 1, 5 and 24, a run longer than one
 * round of the lanes, n_ids of 1 and of 1024, the values at the ends of every dtype -- compared with a restatement of the rule in
 * this file; then the tasks that break a bound, one workgroup per task and one workgroup for all, which must leave the records as
 * they are. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"

extern "C" int emu_png_label_stats_batch(const void *, void *, const debig_png_label_stats_task *, uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Image { uint32_t w, h, n_ids; uint64_t off; std::vector<int64_t> v; };

/* element k of the pattern of image i: blocks of ids, values outside the range among them, the ends of the dtype now and then */
static int64_t value(uint32_t i, uint32_t x, uint32_t y, uint32_t n_ids, uint32_t dtype)
{
    static const int64_t lo[4] = {0, 0, INT32_MIN, INT64_MIN}, hi[4] = {255, 65535, INT32_MAX, INT64_MAX};
    const uint32_t b = (x / 3u + 5u * (y / 2u) + i) * 2654435761u >> 20;
    if (b % 17u == 0) return hi[dtype];
    if (b % 19u == 0) return lo[dtype];
    if (b % 23u == 0) return dtype == 3 ? ((int64_t)1 << 32) + 3 : (int64_t)n_ids;
    if (b % 29u == 0) return dtype >= 2 ? -1 : 255;
    return (int64_t)(b % (n_ids + 1u));
}

/* ... as the dtype holds it */
static int64_t stored(int64_t v, uint32_t dtype)
{
    return dtype == 0 ? (int64_t)(uint8_t)v : dtype == 1 ? (int64_t)(uint16_t)v : dtype == 2 ? (int64_t)(int32_t)v : v;
}

static void put(uint8_t *p, uint32_t dtype, int64_t v)
{
    if (dtype == 0) { const uint8_t q = (uint8_t)v; memcpy(p, &q, 1); }
    else if (dtype == 1) { const uint16_t q = (uint16_t)v; memcpy(p, &q, 2); }
    else if (dtype == 2) { const int32_t q = (int32_t)v; memcpy(p, &q, 4); }
    else memcpy(p, &v, 8);
}

/* the rule, restated: the raw records of one image */
static void restate(const Image &im, std::vector<uint32_t> &raw)
{
    raw.assign((size_t)(im.n_ids + 1u) * 5u, 0u);
    for (uint32_t y = 0; y < im.h; y++)
        for (uint32_t x = 0; x < im.w; x++) {
            const int64_t v = im.v[(size_t)y * im.w + x];
            uint32_t *r = &raw[(size_t)(v >= 0 && v < (int64_t)im.n_ids ? (uint32_t)v : im.n_ids) * 5u];
            r[0]++;
            if (x + 1u > r[1]) r[1] = x + 1u;
            if (y + 1u > r[2]) r[2] = y + 1u;
            if (im.w - x > r[3]) r[3] = im.w - x;
            if (im.h - y > r[4]) r[4] = im.h - y;
        }
}

int main()
{
    static const uint32_t widths[] = {1, 7, 9, 33, 70}, heights[] = {1, 5, 24}, ids[] = {1, 21, 1024};
    for (uint32_t dtype = 0; dtype < 4; dtype++) {
        const uint32_t es = 1u << dtype;
        std::vector<Image> ims;
        uint64_t at = 0, stat_bytes = 0;
        uint32_t k = 0;
        for (uint32_t h : heights)
            for (uint32_t w : widths) ims.push_back({w, h, ids[k++ % 3u], 0, {}});
        ims.push_back({70, 300, 21, 0, {}}); /* 234 rows of it are one task: more than 256 items of every dtype */
        ims.push_back({16384, 1, 6, 0, {}}); /* the widest row */
        for (Image &im : ims) {
            at += (16u - at % 16u) % 16u + es; /* one element behind a multiple of 16 */
            im.off = at;
            at += (uint64_t)im.w * im.h * es;
            stat_bytes += (uint64_t)(im.n_ids + 1u) * 20u;
        }
        uint8_t *labels;
        CHECK(posix_memalign((void **)&labels, 16, at) == 0); /* ends with the last element */
        memset(labels, 0x5A, at);
        for (uint32_t i = 0; i < ims.size(); i++) {
            Image &im = ims[i];
            im.v.resize((size_t)im.w * im.h);
            for (uint32_t y = 0; y < im.h; y++)
                for (uint32_t x = 0; x < im.w; x++) {
                    const int64_t v = stored(value(i, x, y, im.n_ids, dtype), dtype);
                    im.v[(size_t)y * im.w + x] = v;
                    put(labels + im.off + ((uint64_t)y * im.w + x) * es, dtype, v);
                }
        }
        for (uint32_t cut = 0; cut < 3; cut++) /* rows of a task: the host's cut, 4, 1 */
            for (uint32_t grid = 0; grid < 4; grid += (cut == 2 ? 3 : 1)) { /* (row by row through one workgroup per task and through three) */
                std::vector<debig_png_label_stats_task> tasks;
                uint64_t so = 0;
                for (const Image &im : ims) {
                    const uint32_t run = cut == 0 ? (im.w >= DEBIG_PNG_LABEL_STATS_RUN ? 1u : DEBIG_PNG_LABEL_STATS_RUN / im.w) : cut == 1 ? 4u : 1u;
                    for (uint32_t y0 = 0; y0 < im.h; y0 += run) {
                        debig_png_label_stats_task t;
                        memset(&t, 0, sizeof t);
                        t.label_off = im.off + (uint64_t)y0 * im.w * es; t.stat_off = so; t.out_w = im.w; t.out_h = im.h; t.row0 = y0;
                        t.rows = im.h - y0 < run ? im.h - y0 : run; t.n_ids = im.n_ids; t.dtype = dtype;
                        tasks.push_back(t);
                    }
                    so += (uint64_t)(im.n_ids + 1u) * 20u;
                }
                /* (exactly the tasks and exactly the records: heap blocks of their own) */
                debig_png_label_stats_task *tk = (debig_png_label_stats_task *)malloc(tasks.size() * sizeof tasks[0]);
                uint32_t *stats = (uint32_t *)calloc(1, stat_bytes);
                CHECK(tk && stats);
                memcpy(tk, tasks.data(), tasks.size() * sizeof tasks[0]);
                CHECK(emu_png_label_stats_batch(labels, stats, tk, (uint32_t)tasks.size(), grid) == 0);
                so = 0;
                std::vector<uint32_t> raw;
                for (const Image &im : ims) {
                    restate(im, raw);
                    CHECK(memcmp(stats + so / 4u, raw.data(), raw.size() * 4u) == 0);
                    so += (uint64_t)(im.n_ids + 1u) * 20u;
                }
                free(stats);
                free(tk);
            }

        /* the tasks that break a bound, over the 24 x 33 image */
        const Image *g = nullptr;
        for (const Image &im : ims)
            if (im.w == 33 && im.h == 24) g = &im;
        CHECK(g);
        debig_png_label_stats_task good;
        memset(&good, 0, sizeof good);
        good.label_off = g->off; good.out_w = 33; good.out_h = 24; good.rows = 24; good.n_ids = g->n_ids; good.dtype = dtype;
        std::vector<debig_png_label_stats_task> bad(19, good);
        bad[0].dtype = 4; bad[1].dtype = 0xffffffffu; bad[2].n_ids = 0; bad[3].n_ids = 1025; bad[4].n_ids = 0xffffffffu; bad[5].out_w = 0;
        bad[6].out_w = 16385; bad[7].out_h = 0; bad[8].out_h = 16385; bad[9].rows = 0; bad[10].rows = 25; bad[11].row0 = 1;
        bad[12].row0 = 24; bad[13].row0 = 0xffffffffu; bad[14].rows = 0xffffffffu; bad[15].stat_off = 2; bad[16].stat_off = 1;
        bad[17].label_off = g->off + (es > 1 ? 1 : 0); bad[18].label_off = g->off + es / 2u;
        if (es == 1) { bad[17].out_w = 0; bad[18].out_w = 0; } /* (a byte has no misaligned offset) */
        const size_t rec_bytes = (size_t)(g->n_ids + 1u) * 20u;
        for (uint32_t grid = 0; grid < 2; grid++) {
            debig_png_label_stats_task *tk = (debig_png_label_stats_task *)malloc(bad.size() * sizeof bad[0]);
            uint32_t *stats = (uint32_t *)calloc(1, rec_bytes);
            CHECK(tk && stats);
            memcpy(tk, bad.data(), bad.size() * sizeof bad[0]);
            CHECK(emu_png_label_stats_batch(labels, stats, tk, (uint32_t)bad.size(), grid) == 0);
            for (size_t b = 0; b < rec_bytes / 4u; b++) CHECK(stats[b] == 0u);
            free(stats);
            free(tk);
        }
        free(labels);
    }
    puts("asan_png_label_stats_emu: all checks passed");
    return 0;
}
