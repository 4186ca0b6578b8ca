/* DEVELOPMENT / TEST TOOLING: the kernel of level 3 of the PNG encode (csrc/png_encode_lz_kernel.inc) on the CPU lock-step emulator
 * under AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_encode_lz_emu.sh links it with the emulator sources
 * compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * The stream, every slot, every token row and the counts are heap blocks of EXACTLY their sizes (a token row: 4 x chunk_len bytes; a
 * slot: DEBIG_PNG_ENCODE_SLOT(chunk_len)), so a load or a store in front of or behind any of them is ASan's to see -- the bitmaps'
 * look-ahead of 320 positions and the four-byte compares of the table's candidate above all --, and a shift or an index outside its
 * range is UBSan's.  The inputs are the seam and edge ones of the pytest battery (tests/test_emu_png_encode_lz.py): chunk lengths 1,
 * 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1 with bpp 3 and a stride, runs of one byte of 258 .. 600 inside noise
 * from lanes 0, 63 and 1, a run across a chunk seam, rows equal to the row above with the row above in the previous chunk, gp < S,
 * S - bpp = 1, S = 32768 - bpp and no stride, borders shifted by a pixel, a block again at distance 32768 and 32769, noise with a
 * far copy, every flag, under grids 0, 1 and 3.  The output is inflated by the small decoder of tools/asan_png_encode_inflate.h,
 * no task is longer than stored, and every grid gives the same bytes.  Tasks that break a bound must leave every block as it is. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"
#include "asan_png_encode_inflate.h"

typedef debig_png_encode_lz_task ZTask;
extern "C" int emu_png_encode_lz_batch(const void *, void *, void *, const ZTask *, void *, uint32_t, uint32_t);

/* -> the bytes all tasks wrote */
static size_t lz_case(const std::vector<uint8_t> &s, uint32_t bpp, uint32_t stride, uint32_t flags)
{
    const uint32_t C = DEBIG_PNG_ENCODE_CHUNK, nt = (uint32_t)((s.size() + C - 1) / C);
    uint8_t *stream = (uint8_t *)malloc(s.size()); /* exactly its size */
    memcpy(stream, s.data(), s.size());
    std::vector<std::vector<uint8_t>> first;
    size_t total = 0;
    for (uint32_t grid : {0u, 1u, 3u}) {
        /* every slot and every row a heap block of its own: the offsets are relative to the first one's address */
        std::vector<uint8_t *> slots(nt), rows(nt);
        std::vector<ZTask> tasks(nt);
        uint32_t *counts = (uint32_t *)block(4 * (size_t)nt);
        for (uint32_t k = 0; k < nt; k++) {
            const uint32_t len = (uint32_t)(k + 1 == nt ? s.size() - (size_t)k * C : C);
            slots[k] = block((size_t)DEBIG_PNG_ENCODE_SLOT(len));
            rows[k] = block(4 * (size_t)len);
        }
        for (uint32_t k = 0; k < nt; k++) {
            ZTask &t = tasks[grid == 1 ? nt - 1 - k : k]; /* grid 1: the tasks in reversed order */
            memset(&t, 0, sizeof t);
            t.stream_len = s.size(); t.chunk_off = (uint64_t)k * C;
            t.chunk_len = (uint32_t)(k + 1 == nt ? s.size() - (size_t)k * C : C);
            t.slot_cap = (uint32_t)DEBIG_PNG_ENCODE_SLOT(t.chunk_len); t.slot_off = (uint64_t)(slots[k] - slots[0]);
            t.level = 3; t.bpp = bpp; t.last = k + 1 == nt; t.count_idx = k; t.flags = flags;
            t.token_off = (uint64_t)(rows[k] - rows[0]); t.token_cap = 4 * t.chunk_len; t.row_stride = stride;
        }
        CHECK(emu_png_encode_lz_batch(stream, slots[0], rows[0], tasks.data(), counts, nt, grid) == 0);
        std::vector<uint8_t> hist;
        for (uint32_t k = 0; k < nt; k++) {
            const ZTask &t = tasks[grid == 1 ? nt - 1 - k : k];
            const uint32_t n = counts[k];
            CHECK(n > 0 && n <= t.slot_cap);
            if (!flags) CHECK(n <= 5u + t.chunk_len + (t.last ? 0u : 5u)); /* never longer than stored */
            CHECK(untouched(slots[k] + ((n + 3u) & ~3u), t.slot_cap - ((n + 3u) & ~3u)));
            std::vector<uint8_t> win(hist.end() - (hist.size() < 32768 ? hist.size() : 32768), hist.end());
            const size_t before = win.size();
            inflate_task(slots[k], n, win, t.last != 0);
            CHECK(win.size() - before == t.chunk_len && memcmp(win.data() + before, s.data() + t.chunk_off, t.chunk_len) == 0);
            hist.insert(hist.end(), win.begin() + before, win.end());
            std::vector<uint8_t> bytes(slots[k], slots[k] + n);
            if (grid == 0) { first.push_back(bytes); total += n; }
            else CHECK(first[k] == bytes); /* the same bytes for every grid and order */
        }
        CHECK(hist == s);
        for (uint32_t k = 0; k < nt; k++) { free(slots[k]); free(rows[k]); }
        free(counts);
    }
    free(stream);
    return total;
}

static std::vector<uint8_t> noise(size_t n, uint32_t seed, uint32_t lo, uint32_t span)
{
    std::vector<uint8_t> v(n);
    for (auto &b : v) b = (uint8_t)(lo + rnd(seed) % span);
    return v;
}

/* rows of S bytes, each the row above with one byte in `every` changed */
static std::vector<uint8_t> rows_like_above(uint32_t S, uint32_t rows, uint32_t seed, uint32_t every)
{
    std::vector<uint8_t> row = noise(S, seed, 0, 9), s;
    for (uint32_t i = 0; i < S; i++) row[i] = row[i - i % 5];
    for (uint32_t r = 0; r < rows; r++) {
        s.insert(s.end(), row.begin(), row.end());
        for (uint32_t i = rnd(seed) % every; i < S; i += 1 + rnd(seed) % (2 * every)) row[i] = (uint8_t)(rnd(seed) % 9);
    }
    return s;
}

int main()
{
    const uint32_t C = DEBIG_PNG_ENCODE_CHUNK;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)63, (size_t)64, (size_t)65, (size_t)C - 1, (size_t)C, (size_t)C + 1, (size_t)2 * C + 1}) {
        std::vector<uint8_t> s = noise(n, (uint32_t)n, 0, 40);
        for (size_t i = 0; i + 2 < n; i += 3) s[i + 1] = s[i + 2] = s[i]; /* triples: short matches everywhere */
        lz_case(s, 3, 121, 0);
        if (n <= 65) lz_case(s, 1, 0, DEBIG_PNG_ENCODE_ONLY_DYNAMIC);
    }
    for (uint32_t n : {258u, 259u, 321u, 322u, 323u, 384u, 385u, 600u})
        for (uint32_t start : {128u, 127u, 193u, 383u}) { /* the run ends the stream: the look-ahead stands at the block's end */
            std::vector<uint8_t> s = noise(start + n, n + start, 0, 256);
            for (uint32_t i = 0; i < n; i++) s[start + i] = 77;
            lz_case(s, 1, 0, 0);
            s.push_back(78);
            lz_case(s, 2, 100, 0);
        }
    {
        std::vector<uint8_t> s = noise(C - 100, 1, 0, 64);
        s.insert(s.end(), 400, 9);
        s.insert(s.end(), s.begin(), s.begin() + 50);
        lz_case(s, 1, 0, 0); /* a run across the seam */
    }
    {
        const std::vector<uint8_t> a = rows_like_above(1000, 40, 1, 50);
        const size_t with = lz_case(a, 1, 1000, 0), without = lz_case(a, 1, 0, 0); /* the row above lies in the previous chunk; no stride */
        CHECK(with < without);
        lz_case(rows_like_above(700, 3, 2, 50), 3, 700, 0);               /* gp < S on the first row */
        lz_case(rows_like_above(4, 300, 3, 10), 3, 4, 0);                 /* S - bpp = 1 */
        lz_case(rows_like_above(32768 - 4, 2, 4, 1000), 4, 32768 - 4, 0); /* S = 32768 - bpp */
        lz_case(rows_like_above(2, 100, 5, 10), 1, 2, 0);                 /* the smallest stride */
    }
    for (int shift : {-1, 1}) { /* a border that moves one pixel per row */
        const uint32_t W = 300, H = 60;
        std::vector<uint8_t> base = noise(W + 2 * H + 3, 7, 0, 250), s;
        for (size_t i = 0; i < base.size(); i++) base[i] = base[i - i % 3];
        for (uint32_t y = 0; y < H; y++) {
            s.push_back(0);
            for (uint32_t x = 0; x < W; x++) s.push_back(base[(size_t)((int)(H + x) - (int)y * shift)]);
        }
        lz_case(s, 1, 1 + W, 0);
    }
    for (uint32_t period : {32768u, 32769u}) {
        std::vector<uint8_t> blk = noise(300, period, 0, 256), s = blk;
        s.resize(period, 0);
        s.insert(s.end(), blk.begin(), blk.end());
        s.push_back('e');
        lz_case(s, 1, 0, 0);
        std::vector<uint8_t> big = noise(period, period + 1, 0, 64), twice = big;
        twice.insert(twice.end(), big.begin(), big.end());
        lz_case(twice, 4, 32768 - 4, 0);
    }
    {
        std::vector<uint8_t> s = noise(2 * C, 77, 0, 64);
        memcpy(s.data() + C + 31000, s.data() + C + 11000, 200); /* one far copy in noise */
        lz_case(s, 1, 0, 0);
    }
    for (uint32_t flags : {0u, DEBIG_PNG_ENCODE_NO_STORED, DEBIG_PNG_ENCODE_ONLY_DYNAMIC, DEBIG_PNG_ENCODE_NO_STORED | DEBIG_PNG_ENCODE_ONLY_DYNAMIC}) {
        lz_case(noise(C + 500, 2, 144, 112), 1, 50, flags);        /* stored, where the flags allow it */
        lz_case(std::vector<uint8_t>(2 * C + 77, 0), 1, 50, flags); /* fixed beats dynamic */
        lz_case({'a', 'b', 'c', 'X', 'Y', 'Z', 'a', 'b', 'c', 'a', 'b', 'c', 0, 0, 0, 0}, 8, 9, flags);
    }
    /* tasks that break a bound leave every block as it is */
    {
        std::vector<uint8_t> s = noise(1500, 4, 0, 9);
        const size_t cap = (size_t)DEBIG_PNG_ENCODE_SLOT(1500);
        uint8_t *slot = block(cap), *row = block(4 * 1500), *counts = block(4);
        ZTask good;
        memset(&good, 0, sizeof good);
        good.stream_len = 1500; good.chunk_len = 1500; good.slot_cap = (uint32_t)cap; good.level = 3; good.bpp = 3; good.last = 1; good.token_cap = 4 * 1500;
        good.row_stride = 100;
        std::vector<ZTask> bad(18, good);
        bad[0].chunk_len = 0; bad[1].chunk_off = 1500; bad[2].chunk_len = 1501; bad[3].slot_cap -= 16; bad[4].level = 2; bad[5].level = 4; bad[6].last = 2;
        bad[7].bpp = 0; bad[8].bpp = 9; bad[9].slot_off = 2; bad[10].token_off = 2; bad[11].token_cap = 4 * 1500 - 1; bad[12].chunk_len = DEBIG_PNG_ENCODE_CHUNK + 1;
        bad[13].row_stride = 3; bad[14].row_stride = 2; bad[15].row_stride = 32768 - 2; bad[16].row_stride = 0xffffffffu; bad[17].level = 1;
        CHECK(emu_png_encode_lz_batch(s.data(), slot, row, bad.data(), counts, 18, 2) == 0);
        CHECK(untouched(slot, cap) && untouched(row, 4 * 1500) && untouched(counts, 4));
        free(slot); free(row); free(counts);
    }
    printf("all checks passed\n");
    return 0;
}
