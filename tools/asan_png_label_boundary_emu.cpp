/* DEVELOPMENT / TEST TOOLING: the label-boundary kernel (csrc/png_label_boundary_kernel.inc) on the CPU lock-step emulator under
 * AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_label_boundary_emu.sh links it with the emulator sources
 * compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * The labels and the output are heap blocks of exactly their sizes: the label block starts every image one element behind a
 * multiple of 16 bytes and ends with the last element of the last image, the output block likewise, so a load or a store in front
 * of or behind either (a 16-byte store at a row end, a halo read across an image edge) is ASan's to see, and a shift or an index
 * outside its range is UBSan's.  The shapes are the extreme ones of the pytest battery (tests/test_emu_png_label_boundary.py) --
 * 1 x 1, 1 x 7, 9 x 1, widths around the item sizes, an image larger than the largest tile, radii 1, 2, 3, 5 and 16, the three
 * shapes, both modes, tiles of 5 x 3, 32 x 32 and the largest that fit, grids 0 .. 3 -- compared with a brute-force restatement of
 * the rule in this file; then the tasks that break a bound, which must leave the output as it is. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"

extern "C" int emu_png_label_boundary_batch(const void *, void *, const debig_png_label_boundary_task *, uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Image { uint32_t w, h; uint64_t off, out_off; std::vector<int64_t> v; };

/* blocks of ids, the ends of the dtype and values that differ in the high word only among them */
static int64_t value(uint32_t i, uint32_t x, uint32_t y, uint32_t dtype)
{
    static const int64_t lo[4] = {0, 0, INT32_MIN, INT64_MIN}, hi[4] = {255, 65535, INT32_MAX, INT64_MAX};
    const uint32_t b = (x / 6u + 5u * (y / 4u) + i) * 2654435761u >> 20;
    if (b % 17u == 0) return hi[dtype];
    if (b % 19u == 0) return lo[dtype];
    if (b % 23u == 0) return dtype == 3 ? ((int64_t)1 << 32) + 3 : 3;
    return (int64_t)(b % 5u);
}

static void put(uint8_t *p, uint32_t es, int64_t v) { memcpy(p, &v, es); } /* (little endian: the low bytes) */

static int64_t stored(int64_t v, uint32_t dtype)
{
    return dtype == 0 ? (int64_t)(uint8_t)v : dtype == 1 ? (int64_t)(uint16_t)v : dtype == 2 ? (int64_t)(int32_t)v : v;
}

/* reach[0 .. r] of shape 0 square, 1 diamond, 2 disk */
static void reach_of(uint32_t r, uint32_t shape, uint8_t reach[17])
{
    memset(reach, 0, 17);
    for (uint32_t d = 0; d <= r; d++) {
        uint32_t v = r;
        if (shape == 1) v = r - d;
        if (shape == 2) while (v * v + d * d > r * r) v--;
        reach[d] = (uint8_t)v;
    }
}

/* the rule by brute force */
static bool boundary(const Image &im, uint32_t x, uint32_t y, uint32_t r, const uint8_t reach[17])
{
    const int64_t v = im.v[(size_t)y * im.w + x];
    for (int32_t dy = -(int32_t)r; dy <= (int32_t)r; dy++) {
        const int32_t yy = (int32_t)y + dy, rx = reach[dy < 0 ? -dy : dy];
        if (yy < 0 || yy >= (int32_t)im.h) continue;
        for (int32_t dx = -rx; dx <= rx; dx++) {
            const int32_t xx = (int32_t)x + dx;
            if (xx >= 0 && xx < (int32_t)im.w && im.v[(size_t)yy * im.w + xx] != v) return true;
        }
    }
    return false;
}

int main()
{
    static const uint32_t sizes[][2] = {{1, 1}, {7, 1}, {1, 9}, {15, 5}, {16, 3}, {17, 24}, {33, 24}, {70, 40}, {200, 70}};
    static const uint32_t radii[] = {1, 2, 3, 5, 16};
    static const int64_t ring_value[4] = {255, 65535, INT32_MIN, INT64_MAX};
    for (uint32_t dtype = 0; dtype < 4; dtype++)
        for (uint32_t mode = 0; mode < 2; mode++) {
            const uint32_t es = 1u << dtype, os = mode ? 1u : es;
            std::vector<Image> ims;
            uint64_t at = 0, ot = 0;
            for (const uint32_t *s : sizes) ims.push_back({s[0], s[1], 0, 0, {}});
            for (Image &im : ims) {
                at += (16u - at % 16u) % 16u + es; /* one element behind a multiple of 16 */
                ot += (16u - ot % 16u) % 16u + os;
                im.off = at;
                im.out_off = ot;
                at += (uint64_t)im.w * im.h * es;
                ot += (uint64_t)im.w * im.h * os;
            }
            uint8_t *labels;
            CHECK(posix_memalign((void **)&labels, 16, at) == 0); /* ends with the last element */
            memset(labels, 0x5A, at);
            for (uint32_t i = 0; i < ims.size(); i++) {
                Image &im = ims[i];
                im.v.resize((size_t)im.w * im.h);
                for (uint32_t y = 0; y < im.h; y++)
                    for (uint32_t x = 0; x < im.w; x++) {
                        const int64_t v = stored(value(i, x, y, dtype), dtype);
                        im.v[(size_t)y * im.w + x] = v;
                        put(labels + im.off + ((uint64_t)y * im.w + x) * es, es, v);
                    }
            }
            uint32_t round = 0;
            for (uint32_t r : radii)
                for (uint32_t shape = 0; shape < 3; shape++, round++) {
                    uint8_t reach[17];
                    reach_of(r, shape, reach);
                    uint32_t tw = 128, th = 64; /* the host's cut, 32 x 32, 5 x 3 in turn */
                    while (DEBIG_PNG_LABEL_BOUNDARY_TILE_BYTES(tw, th, dtype, r) > DEBIG_PNG_LABEL_BOUNDARY_LDS_BYTES) {
                        if (tw > th) tw /= 2; else th /= 2;
                    }
                    if (round % 3u == 1) tw = th = 32;
                    if (round % 3u == 2) { tw = 5; th = 3; }
                    std::vector<debig_png_label_boundary_task> tasks;
                    for (const Image &im : ims) {
                        if (tw == 5 && im.w > 70) continue; /* (thousands of tiny tiles prove nothing more) */
                        for (uint32_t y0 = 0; y0 < im.h; y0 += th)
                            for (uint32_t x0 = 0; x0 < im.w; x0 += tw) {
                                debig_png_label_boundary_task t;
                                memset(&t, 0, sizeof t);
                                t.label_off = im.off; t.out_off = im.out_off; t.value = ring_value[dtype]; t.w = im.w; t.h = im.h;
                                t.x0 = x0; t.y0 = y0; t.tile_w = im.w - x0 < tw ? im.w - x0 : tw; t.tile_h = im.h - y0 < th ? im.h - y0 : th;
                                t.dtype = dtype; t.mode = mode; t.radius = r;
                                memcpy(t.reach, reach, 17);
                                tasks.push_back(t);
                            }
                    }
                    /* (exactly the tasks and exactly the output: heap blocks of their own) */
                    debig_png_label_boundary_task *tk = (debig_png_label_boundary_task *)malloc(tasks.size() * sizeof tasks[0]);
                    uint8_t *out;
                    CHECK(posix_memalign((void **)&out, 16, ot) == 0 && tk);
                    memset(out, 0xEE, ot);
                    memcpy(tk, tasks.data(), tasks.size() * sizeof tasks[0]);
                    CHECK(emu_png_label_boundary_batch(labels, out, tk, (uint32_t)tasks.size(), round % 4u) == 0);
                    for (const Image &im : ims) {
                        if (tw == 5 && im.w > 70) continue;
                        for (uint32_t y = 0; y < im.h; y++)
                            for (uint32_t x = 0; x < im.w; x++) {
                                const bool b = boundary(im, x, y, r, reach);
                                const int64_t exp = mode ? (int64_t)b : b ? ring_value[dtype] : im.v[(size_t)y * im.w + x];
                                CHECK(memcmp(out + im.out_off + ((uint64_t)y * im.w + x) * os, &exp, os) == 0);
                            }
                    }
                    free(out);
                    free(tk);
                }

            /* the tasks that break a bound, over the 33 x 24 image as one tile */
            const Image *g = nullptr;
            for (const Image &im : ims)
                if (im.w == 33 && im.h == 24) g = &im;
            CHECK(g);
            debig_png_label_boundary_task good;
            memset(&good, 0, sizeof good);
            good.label_off = g->off; good.out_off = g->out_off; good.value = 1; good.w = 33; good.h = 24; good.tile_w = 33; good.tile_h = 24;
            good.dtype = dtype; good.mode = mode; good.radius = 2;
            reach_of(2, 0, good.reach);
            std::vector<debig_png_label_boundary_task> bad(24, good);
            bad[0].dtype = 4; bad[1].dtype = 0xffffffffu; bad[2].mode = 2; bad[3].radius = 0; bad[4].radius = 17; bad[5].reach[1] = 3;
            bad[6].w = 0; bad[7].w = 16385; bad[8].h = 0; bad[9].h = 16385; bad[10].tile_w = 0; bad[11].tile_h = 0; bad[12].tile_w = 34;
            bad[13].tile_h = 25; bad[14].x0 = 1; bad[15].y0 = 1; bad[16].x0 = 0xffffffffu; bad[17].y0 = 0xffffffffu;
            bad[18].tile_w = 0xffffffffu; bad[19].tile_h = DEBIG_PNG_LABEL_BOUNDARY_MAX_TILE + 1u;
            bad[20].label_off = g->off + es / 2u; bad[21].out_off = g->out_off + os / 2u;
            if (es == 1) bad[20].w = 0; /* (a byte has no misaligned offset) */
            if (os == 1) bad[21].w = 0;
            bad[22].value = mode ? 0 : dtype == 0 ? 256 : dtype == 1 ? -1 : dtype == 2 ? (int64_t)INT32_MAX + 1 : 0;
            if (mode || dtype == 3) bad[22].w = 0; /* (every value fits an int64; EDGE does not look at it) */
            bad[23].radius = 0xffffffffu;
            for (uint32_t grid = 0; grid < 2; grid++) {
                debig_png_label_boundary_task *tk = (debig_png_label_boundary_task *)malloc(bad.size() * sizeof bad[0]);
                uint8_t *out = (uint8_t *)malloc(ot);
                CHECK(tk && out);
                memset(out, 0xEE, ot);
                memcpy(tk, bad.data(), bad.size() * sizeof bad[0]);
                CHECK(emu_png_label_boundary_batch(labels, out, tk, (uint32_t)bad.size(), grid) == 0);
                for (uint64_t b = 0; b < ot; b++) CHECK(out[b] == 0xEE);
                free(out);
                free(tk);
            }
            free(labels);
        }
    puts("asan_png_label_boundary_emu: all checks passed");
    return 0;
}
