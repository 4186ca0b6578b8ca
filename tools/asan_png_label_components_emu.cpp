/* DEVELOPMENT / TEST TOOLING: the five label-components kernels (csrc/png_label_components_kernel.inc) on the CPU lock-step emulator
 * under AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_label_components_emu.sh links it with the emulator
 * sources compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing
 * preloaded).
 *
 * The labels, the parent planes, the counts and the output are heap blocks of exactly their sizes: every image starts one element
 * behind a multiple of 16 bytes and the block ends with the last element of the last image, so a load or a store in front of or
 * behind any of them (the row above a task's first row, the neighbours of a row's first and last element, a slot that a wrong index
 * names) is ASan's to see, and a shift or an index outside its range is UBSan's.  The shapes are the extreme ones of the pytest
 * battery (tests/test_emu_png_label_components.py) -- 1 x 1, 1 x 7, 9 x 1, widths around the segment size, a checkerboard, a
 * serpentine, 16384 x 1, 1 x 16384, 5000 x 3, both connectivities, with and without a background, both id modes, cuts and grids --
 * compared with a flood fill in this file; then parent planes that hold anything (the launches behind rows must end and stay inside
 * their blocks), and the tasks that break a bound, which must leave every block as it is.  The emulator runs the workgroups one after
 * the other: this shows the rule and the bounds, not the races. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"

typedef debig_png_label_components_task Task;
extern "C" int emu_png_label_components_rows_batch(const void *, void *, const Task *, uint32_t, uint32_t);
extern "C" int emu_png_label_components_merge_batch(const void *, void *, const Task *, uint32_t, uint32_t);
extern "C" int emu_png_label_components_count_batch(const void *, void *, const Task *, uint32_t, uint32_t);
extern "C" int emu_png_label_components_number_batch(const void *, const void *, void *, const Task *, uint32_t, uint32_t);
extern "C" int emu_png_label_components_finish_batch(const void *, void *, const Task *, uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Image { uint32_t w, h, kind; uint64_t off, p_off, out_off; uint32_t word0, n_tasks; std::vector<int64_t> v; };

/* kind 0: blocks of ids with the ends of the dtype and values that differ in the high word only among them; 1: a checkerboard;
 * 2: a serpentine of ones (corridors in every other row, joined at alternating ends); 3: runs of 37 along the raster */
static int64_t value(const Image &im, uint32_t i, uint32_t x, uint32_t y, uint32_t dtype)
{
    static const int64_t lo[4] = {0, 0, INT32_MIN, INT64_MIN}, hi[4] = {255, 65535, INT32_MAX, INT64_MAX};
    if (im.kind == 1) return (x + y) % 2u;
    if (im.kind == 2) return y % 2u == 0 ? 1 : (x == ((y / 2u) % 2u == 0 ? im.w - 1u : 0u) ? 1 : 0);
    if (im.kind == 3) return (((uint64_t)y * im.w + x) / 37u * 2654435761u >> 13) % 2u;
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

/* the rule by flood fill from every unvisited element in raster order -> FIRST per element (-1: background), and K */
static uint32_t flood(const Image &im, uint32_t connectivity, bool use_bg, int64_t bg, std::vector<int32_t> &first)
{
    const uint32_t W = im.w, H = im.h;
    first.assign((size_t)W * H, -2);
    std::vector<uint32_t> stack;
    uint32_t k = 0;
    for (uint32_t s = 0; s < W * H; s++) {
        if (first[s] != -2) continue;
        if (use_bg && im.v[s] == bg) { first[s] = -1; continue; }
        k++;
        first[s] = (int32_t)s;
        stack.push_back(s);
        while (!stack.empty()) {
            const uint32_t p = stack.back(), x = p % W, y = p / W;
            stack.pop_back();
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if ((dx == 0 && dy == 0) || (connectivity == 4 && dx != 0 && dy != 0)) continue;
                    const int64_t xx = (int64_t)x + dx, yy = (int64_t)y + dy;
                    if (xx < 0 || yy < 0 || xx >= W || yy >= H) continue;
                    const uint32_t q = (uint32_t)yy * W + (uint32_t)xx;
                    if (first[q] != -2 || im.v[q] != im.v[p]) continue;
                    first[q] = (int32_t)s;
                    stack.push_back(q);
                }
        }
    }
    return k;
}

template <typename T> static T *exact(const std::vector<T> &v)
{
    T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    CHECK(p);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int main()
{
    static const uint32_t shapes[][3] = {{1, 1, 0}, {7, 1, 0}, {1, 9, 0}, {63, 5, 0}, {64, 3, 0}, {65, 24, 0}, {33, 24, 0}, {70, 40, 0},
                                         {23, 17, 1}, {13, 21, 2}, {2, 5, 1}, {16384, 1, 3}, {1, 16384, 3}, {5000, 3, 3}};
    uint32_t round = 0;
    for (uint32_t dtype = 0; dtype < 4; dtype++) {
        const uint32_t es = 1u << dtype;
        std::vector<Image> ims;
        uint64_t at = 0, pt = 0, ot = 0;
        for (const uint32_t *s : shapes)
            if (s[2] < 3 || dtype == 0) ims.push_back({s[0], s[1], s[2], 0, 0, 0, 0, 0, {}}); /* (the long images once: uint8) */
        for (Image &im : ims) {
            at += (16u - at % 16u) % 16u + es; /* one element behind a multiple of 16 */
            pt += (16u - pt % 16u) % 16u + 4u;
            ot += (16u - ot % 16u) % 16u + 4u;
            im.off = at;
            im.p_off = pt;
            im.out_off = ot;
            at += (uint64_t)im.w * im.h * es;
            pt += (uint64_t)im.w * im.h * 4u;
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
        /* no background, a present one, one that the dtype cannot hold (int64: an absent one) */
        const int64_t bgs[3] = {0, 1, dtype == 0 ? 257 : dtype == 1 ? 65537 : dtype == 2 ? ((int64_t)1 << 32) + 1 : 77};
        for (uint32_t connectivity = 4; connectivity <= 8; connectivity += 4)
            for (uint32_t b = 0; b < 3; b++)
                for (uint32_t ids = 0; ids < 2; ids++)
                    for (uint32_t spoilt = 0; spoilt < 2; spoilt++, round++) {
                        std::vector<Task> ts;
                        for (Image &im : ims) {
                            uint32_t run = im.w >= DEBIG_PNG_LABEL_COMPONENTS_ELEMS ? 1u : DEBIG_PNG_LABEL_COMPONENTS_ELEMS / im.w;
                            if (round % 2u && im.h <= 40 && im.w <= 70) run = 1u + round % 5u; /* the host's cut and short runs in turn */
                            im.word0 = (uint32_t)ts.size();
                            for (uint32_t y0 = 0; y0 < im.h; y0 += run) {
                                Task t;
                                memset(&t, 0, sizeof t);
                                t.label_off = im.off; t.parent_off = im.p_off; t.out_off = im.out_off; t.background = bgs[b];
                                t.w = im.w; t.h = im.h; t.row0 = y0; t.rows = im.h - y0 < run ? im.h - y0 : run; t.dtype = dtype;
                                t.connectivity = connectivity; t.use_background = b != 0; t.ids = ids;
                                t.count_idx = (uint32_t)ts.size(); t.count_first = im.word0;
                                ts.push_back(t);
                            }
                            im.n_tasks = (uint32_t)ts.size() - im.word0;
                        }
                        /* (exactly the tasks, the planes, the counts and the output: heap blocks of their own) */
                        Task *tk = exact(ts);
                        const uint32_t n = (uint32_t)ts.size();
                        uint8_t *parent, *out;
                        uint32_t *counts = (uint32_t *)malloc((size_t)n * 4u);
                        CHECK(posix_memalign((void **)&parent, 16, pt) == 0 && posix_memalign((void **)&out, 16, ot) == 0 && counts);
                        memset(parent, 0xEE, pt);
                        memset(out, 0xEE, ot);
                        memset(counts, 0xEE, (size_t)n * 4u);
                        CHECK(emu_png_label_components_rows_batch(labels, parent, tk, n, round % 4u) == 0);
                        if (spoilt) /* a plane that holds anything: out of range, above the slot, inside the image */
                            for (const Image &im : ims) {
                                uint32_t *pp = (uint32_t *)(parent + im.p_off), s = round * 2654435761u + 12345u;
                                for (uint32_t p = 0; p < im.w * im.h; p++) {
                                    s = s * 1664525u + 1013904223u;
                                    pp[p] = round % 3u == 0 ? s : round % 3u == 1 ? p + 1u + (s >> 29) : (s >> 8) % (im.w * im.h);
                                }
                            }
                        CHECK(emu_png_label_components_merge_batch(labels, parent, tk, n, round % 3u) == 0);
                        CHECK(emu_png_label_components_count_batch(parent, counts, tk, n, round % 5u) == 0);
                        if (ids) CHECK(emu_png_label_components_number_batch(parent, counts, out, tk, n, round % 4u) == 0);
                        CHECK(emu_png_label_components_finish_batch(parent, out, tk, n, round % 2u) == 0);
                        if (!spoilt) {
                            std::vector<int32_t> first;
                            for (const Image &im : ims) {
                                const bool holds = dtype == 3 || b != 2; /* (the third background is one nothing can equal, or absent) */
                                const uint32_t K = flood(im, connectivity, b != 0 && holds, bgs[b], first);
                                uint32_t sum = 0, seen = 0;
                                for (uint32_t k = 0; k < im.n_tasks; k++) sum += counts[im.word0 + k];
                                CHECK(sum == K);
                                for (uint32_t p = 0; p < im.w * im.h; p++) {
                                    int32_t exp = first[p];
                                    if (first[p] == (int32_t)p) seen++;
                                    if (ids) exp = first[p] < 0 ? 0 : -3; /* (numbered below) */
                                    int32_t got;
                                    memcpy(&got, out + im.out_off + (uint64_t)p * 4u, 4);
                                    if (ids && first[p] == (int32_t)p) CHECK(got == (int32_t)seen);
                                    else if (ids && first[p] >= 0) {
                                        int32_t of_first;
                                        memcpy(&of_first, out + im.out_off + (uint64_t)first[p] * 4u, 4);
                                        CHECK(got == of_first && got >= 1);
                                    } else CHECK(got == exp);
                                }
                                CHECK(seen == K);
                            }
                        }
                        free(out);
                        free(parent);
                        free(counts);
                        free(tk);
                    }

        /* the tasks that break a bound, over the 33 x 24 image as one run of rows */
        const Image *gi = nullptr;
        for (const Image &im : ims)
            if (im.w == 33 && im.h == 24) gi = &im;
        CHECK(gi);
        Task good;
        memset(&good, 0, sizeof good);
        good.label_off = gi->off; good.parent_off = gi->p_off; good.out_off = gi->out_off; good.w = 33; good.h = 24; good.rows = 24;
        good.dtype = dtype; good.connectivity = 8; good.ids = 1;
        std::vector<Task> bad(24, good);
        bad[0].dtype = 4; bad[1].dtype = 0xffffffffu; bad[2].connectivity = 0; bad[3].connectivity = 6; bad[4].use_background = 2;
        bad[5].ids = 2; bad[6].w = 0; bad[7].w = 16385; bad[8].h = 0; bad[9].h = 16385; bad[10].rows = 0; bad[11].rows = 25;
        bad[12].row0 = 1; bad[13].row0 = 24; bad[14].row0 = 0xffffffffu; bad[15].rows = 0xffffffffu; bad[16].parent_off = gi->p_off + 2;
        bad[17].out_off = gi->out_off + 1; bad[18].label_off = gi->off + es / 2u;
        if (es == 1) bad[18].w = 0; /* (a byte has no misaligned offset) */
        bad[19].w = 1000; bad[19].h = 1000; bad[19].rows = 17; /* more than 16384 elements in more than one row */
        bad[20].count_first = 1; bad[21].count_idx = 16384; bad[22].connectivity = 0xfffffffcu; bad[23].ids = 0x80000000u;
        for (uint32_t grid = 0; grid < 2; grid++) {
            Task *tk = exact(bad);
            const uint32_t n = (uint32_t)bad.size();
            uint8_t *parent = (uint8_t *)malloc(pt), *out = (uint8_t *)malloc(ot);
            uint32_t *counts = (uint32_t *)malloc(4);
            CHECK(parent && out && counts);
            memset(parent, 0xEE, pt);
            memset(out, 0xEE, ot);
            memset(counts, 0xEE, 4);
            CHECK(emu_png_label_components_rows_batch(labels, parent, tk, n, grid) == 0);
            CHECK(emu_png_label_components_merge_batch(labels, parent, tk, n, grid) == 0);
            CHECK(emu_png_label_components_count_batch(parent, counts, tk, n, grid) == 0);
            CHECK(emu_png_label_components_number_batch(parent, counts, out, tk, n, grid) == 0);
            CHECK(emu_png_label_components_finish_batch(parent, out, tk, n, grid) == 0);
            for (uint64_t b = 0; b < pt; b++) CHECK(parent[b] == 0xEE);
            for (uint64_t b = 0; b < ot; b++) CHECK(out[b] == 0xEE);
            CHECK(counts[0] == 0xEEEEEEEEu);
            free(out);
            free(parent);
            free(counts);
            free(tk);
        }
        free(labels);
    }
    puts("asan_png_label_components_emu: all checks passed");
    return 0;
}
