/* DEVELOPMENT / TEST TOOLING: the two kernels of level 2 of the PNG encode (csrc/png_encode_dynamic_kernel.inc) on the CPU lock-step
 * emulator under AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_encode_dyn_emu.sh links it with the emulator
 * sources compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing
 * preloaded).
 *
 * The stream, every slot, every token row, the counts, the histograms and the length lists are heap blocks of EXACTLY their sizes
 * (a token row: 4 x chunk_len bytes; a slot: DEBIG_PNG_ENCODE_SLOT(chunk_len)), so a load or a store in front of or behind any of
 * them is ASan's to see, and a shift or an index outside its range is UBSan's.  The inputs are the seam and edge ones of the pytest
 * battery (tests/test_emu_png_encode_dyn.py): chunk lengths 1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1, 600 equal
 * bytes, all 256 values once, two values only, a run across a chunk seam, a block again at distance 32768 and 32769, noise with a
 * far copy, every flag, under grids 0, 1 and 3.  The output is inflated by a small decoder in this file (all three block types; a
 * match may reach into the 32768 bytes in front of the chunk and nowhere else), level 2 is never longer than level 1, and the codes
 * kernel's lengths are complete and within the limit.  Tasks that break a bound must leave every block as it is. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"
#include "asan_png_encode_inflate.h"

typedef debig_png_encode_deflate_task DTask;
typedef debig_png_encode_dynamic_task YTask;
typedef debig_png_encode_codes_task CTask;
extern "C" int emu_png_encode_deflate_batch(const void *, void *, const DTask *, void *, uint32_t, uint32_t);
extern "C" int emu_png_encode_dynamic_batch(const void *, void *, void *, const YTask *, void *, uint32_t, uint32_t);
extern "C" int emu_png_encode_codes_batch(const void *, void *, const CTask *, uint32_t, uint32_t);

/* -> how many tasks wrote a dynamic block */
static uint32_t dynamic_case(const std::vector<uint8_t> &s, uint32_t bpp, uint32_t flags)
{
    const uint32_t C = DEBIG_PNG_ENCODE_CHUNK, nt = (uint32_t)((s.size() + C - 1) / C);
    uint8_t *stream = (uint8_t *)malloc(s.size()); /* exactly its size */
    memcpy(stream, s.data(), s.size());
    std::vector<std::vector<uint8_t>> first;
    uint32_t n_dyn = 0;
    for (uint32_t grid : {0u, 1u, 3u}) {
        /* every slot and every row a heap block of its own: the offsets are relative to the first one's address */
        std::vector<uint8_t *> slots(nt), rows(nt), slots1(nt);
        std::vector<YTask> tasks(nt);
        std::vector<DTask> tasks1(nt);
        uint32_t *counts = (uint32_t *)block(4 * (size_t)nt), *counts1 = (uint32_t *)block(4 * (size_t)nt);
        for (uint32_t k = 0; k < nt; k++) {
            const uint32_t len = (uint32_t)(k + 1 == nt ? s.size() - (size_t)k * C : C);
            slots[k] = block((size_t)DEBIG_PNG_ENCODE_SLOT(len));
            slots1[k] = block((size_t)DEBIG_PNG_ENCODE_SLOT(len));
            rows[k] = block(4 * (size_t)len);
        }
        for (uint32_t k = 0; k < nt; k++) {
            YTask &t = tasks[grid == 1 ? nt - 1 - k : k]; /* grid 1: the tasks in reversed order */
            memset(&t, 0, sizeof t);
            t.stream_len = s.size(); t.chunk_off = (uint64_t)k * C;
            t.chunk_len = (uint32_t)(k + 1 == nt ? s.size() - (size_t)k * C : C);
            t.slot_cap = (uint32_t)DEBIG_PNG_ENCODE_SLOT(t.chunk_len); t.slot_off = (uint64_t)(slots[k] - slots[0]);
            t.level = 2; t.bpp = bpp; t.last = k + 1 == nt; t.count_idx = k; t.flags = flags;
            t.token_off = (uint64_t)(rows[k] - rows[0]); t.token_cap = 4 * t.chunk_len;
            DTask &t1 = tasks1[k];
            memcpy(&t1, &t, sizeof t1);
            t1.level = 1; t1.flags = flags & DEBIG_PNG_ENCODE_NO_STORED; t1.slot_off = (uint64_t)(slots1[k] - slots1[0]);
        }
        CHECK(emu_png_encode_dynamic_batch(stream, slots[0], rows[0], tasks.data(), counts, nt, grid) == 0);
        CHECK(emu_png_encode_deflate_batch(stream, slots1[0], tasks1.data(), counts1, nt, grid) == 0);
        std::vector<uint8_t> hist;
        for (uint32_t k = 0; k < nt; k++) {
            const YTask &t = tasks[grid == 1 ? nt - 1 - k : k];
            const uint32_t n = counts[k];
            CHECK(n > 0 && n <= t.slot_cap);
            if (!(flags & DEBIG_PNG_ENCODE_ONLY_DYNAMIC)) CHECK(n <= counts1[k]); /* level 2 <= level 1 */
            CHECK(untouched(slots[k] + ((n + 3u) & ~3u), t.slot_cap - ((n + 3u) & ~3u)));
            std::vector<uint8_t> win(hist.end() - (hist.size() < 32768 ? hist.size() : 32768), hist.end());
            const size_t before = win.size();
            const uint32_t bt = inflate_task(slots[k], n, win, t.last != 0);
            if (grid == 0 && bt == 2) n_dyn++;
            if (bt != 2) CHECK(n == counts1[k] && memcmp(slots[k], slots1[k], n) == 0); /* what level 1 writes */
            CHECK(win.size() - before == t.chunk_len && memcmp(win.data() + before, s.data() + t.chunk_off, t.chunk_len) == 0);
            hist.insert(hist.end(), win.begin() + before, win.end());
            std::vector<uint8_t> bytes(slots[k], slots[k] + n);
            if (grid == 0) first.push_back(bytes);
            else CHECK(first[k] == bytes); /* the same bytes for every grid and order */
        }
        CHECK(hist == s);
        for (uint32_t k = 0; k < nt; k++) { free(slots[k]); free(slots1[k]); free(rows[k]); }
        free(counts);
        free(counts1);
    }
    free(stream);
    return n_dyn;
}

static std::vector<uint8_t> noise(size_t n, uint32_t seed, uint32_t lo, uint32_t span)
{
    std::vector<uint8_t> v(n);
    for (auto &b : v) b = (uint8_t)(lo + rnd(seed) % span);
    return v;
}

static void codes_case(const std::vector<uint32_t> &c, uint32_t limit, uint32_t grid)
{
    uint32_t *counts = (uint32_t *)malloc(4 * c.size()); /* exactly their sizes */
    memcpy(counts, c.data(), 4 * c.size());
    uint8_t *lens = block(c.size());
    CTask t = {0, 0, (uint32_t)c.size(), limit};
    CTask two[2] = {t, t};
    CHECK(emu_png_encode_codes_batch(counts, lens, two, 2, grid) == 0);
    uint32_t used = 0, ones = 0;
    uint64_t kraft = 0;
    for (size_t s = 0; s < c.size(); s++) {
        CHECK(lens[s] <= limit);
        used += c[s] != 0;
        ones += lens[s] == 1;
        if (lens[s]) kraft += 1ull << (limit - lens[s]);
    }
    if (used >= 2) {
        CHECK(kraft == 1ull << limit);
        for (size_t s = 0; s < c.size(); s++) CHECK((lens[s] != 0) == (c[s] != 0));
    } else CHECK(ones == (c.size() < 2 ? c.size() : 2));
    free(counts);
    free(lens);
}

int main()
{
    const uint32_t C = DEBIG_PNG_ENCODE_CHUNK;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)63, (size_t)64, (size_t)65, (size_t)C - 1, (size_t)C, (size_t)C + 1, (size_t)2 * C + 1}) {
        std::vector<uint8_t> s = noise(n, (uint32_t)n, 0, 40);
        for (size_t i = 0; i + 2 < n; i += 3) s[i + 1] = s[i + 2] = s[i]; /* triples: short matches everywhere */
        const uint32_t nd = dynamic_case(s, 3, 0);
        if (n >= 63) CHECK(nd >= 1);
        if (n <= 65) CHECK(dynamic_case(s, 1, DEBIG_PNG_ENCODE_ONLY_DYNAMIC) == 1);
    }
    CHECK(dynamic_case(std::vector<uint8_t>(600, 7), 1, DEBIG_PNG_ENCODE_ONLY_DYNAMIC) == 1); /* one distance symbol */
    {
        std::vector<uint8_t> all(256);
        for (uint32_t i = 0; i < 256; i++) all[i] = (uint8_t)i;
        CHECK(dynamic_case(all, 1, DEBIG_PNG_ENCODE_ONLY_DYNAMIC) == 1); /* flat lengths */
        std::vector<uint8_t> many(57); /* 57 different bytes: a block of 98 bytes, a slot of 96 */
        for (uint32_t i = 0; i < 57; i++) many[i] = (uint8_t)(255 - 4 * i);
        CHECK(dynamic_case(many, 1, DEBIG_PNG_ENCODE_ONLY_DYNAMIC) == 0); /* a dynamic block that does not fit its slot */
        CHECK(dynamic_case(many, 1, DEBIG_PNG_ENCODE_ONLY_DYNAMIC | DEBIG_PNG_ENCODE_NO_STORED) == 0);
    }
    {
        std::vector<uint8_t> two = noise(3000, 6, 0, 2);
        for (auto &b : two) b = (uint8_t)(b * 199 + 3);
        CHECK(dynamic_case(two, 1, 0) == 1); /* long zero runs in the header */
        CHECK(dynamic_case(two, 1, DEBIG_PNG_ENCODE_NO_STORED) == 1);
    }
    {
        std::vector<uint8_t> s = noise(C - 100, 1, 0, 64);
        s.insert(s.end(), 400, 9);
        s.insert(s.end(), s.begin(), s.begin() + 50);
        CHECK(dynamic_case(s, 1, 0) >= 1); /* a run across the seam */
    }
    for (uint32_t period : {32768u, 32769u}) {
        std::vector<uint8_t> blk = noise(300, period, 0, 256), s = blk;
        s.resize(period, 0);
        s.insert(s.end(), blk.begin(), blk.end());
        s.push_back('e');
        dynamic_case(s, 1, 0);
        std::vector<uint8_t> big = noise(period, period + 1, 0, 64), twice = big;
        twice.insert(twice.end(), big.begin(), big.end());
        dynamic_case(twice, 4, 0);
    }
    {
        std::vector<uint8_t> s = noise(2 * C, 77, 0, 64);
        memcpy(s.data() + C + 31000, s.data() + C + 11000, 200); /* one far copy in noise */
        CHECK(dynamic_case(s, 1, 0) == 2);
    }
    dynamic_case(noise(C + 500, 2, 144, 112), 1, 0);                 /* stored */
    dynamic_case(std::vector<uint8_t>(2 * C + 77, 0), 1, 0);          /* fixed beats dynamic */
    dynamic_case({'a', 'b', 'c', 'X', 'Y', 'Z', 'a', 'b', 'c', 'a', 'b', 'c', 0, 0, 0, 0}, 8, 0);
    /* the code builder */
    {
        std::vector<uint32_t> f20 = {1, 1}, f10;
        while (f20.size() < 20) f20.push_back(f20[f20.size() - 1] + f20[f20.size() - 2]);
        f10.assign(f20.begin(), f20.begin() + 10);
        for (uint32_t grid : {0u, 1u}) {
            codes_case(f20, 15, grid);
            codes_case(f10, 7, grid);
            codes_case(std::vector<uint32_t>(286, 7), 15, grid);
            codes_case(std::vector<uint32_t>(286, 32768), 15, grid);
            codes_case(std::vector<uint32_t>(286, DEBIG_PNG_ENCODE_CODES_MAX_COUNT), 15, grid);
            codes_case(std::vector<uint32_t>(30, 0), 15, grid);
            codes_case(std::vector<uint32_t>(19, 0), 7, grid);
            std::vector<uint32_t> far(286, 0), one(30, 0);
            far[0] = 5; far[285] = 9; one[17] = 4;
            codes_case(far, 15, grid);
            codes_case(one, 15, grid);
            codes_case({3}, 1, grid);
            uint32_t seed = 9 + grid;
            for (uint32_t k = 0; k < 40; k++) {
                const uint32_t n = k % 3 == 0 ? 286 : k % 3 == 1 ? 30 : 19;
                std::vector<uint32_t> c(n);
                for (auto &v : c) v = rnd(seed) % 4 == 0 ? 0 : rnd(seed) >> (8 + rnd(seed) % 16);
                codes_case(c, n == 19 ? 7 : 15, grid);
            }
        }
    }
    /* tasks that break a bound leave every block as it is */
    {
        std::vector<uint8_t> s = noise(1500, 4, 0, 9);
        const size_t cap = (size_t)DEBIG_PNG_ENCODE_SLOT(1500);
        uint8_t *slot = block(cap), *row = block(4 * 1500), *counts = block(4);
        YTask good;
        memset(&good, 0, sizeof good);
        good.stream_len = 1500; good.chunk_len = 1500; good.slot_cap = (uint32_t)cap; good.level = 2; good.bpp = 1; good.last = 1; good.token_cap = 4 * 1500;
        std::vector<YTask> bad(13, good);
        bad[0].chunk_len = 0; bad[1].chunk_off = 1500; bad[2].chunk_len = 1501; bad[3].slot_cap -= 16; bad[4].level = 1; bad[5].level = 3; bad[6].last = 2;
        bad[7].bpp = 0; bad[8].bpp = 9; bad[9].slot_off = 2; bad[10].token_off = 2; bad[11].token_cap = 4 * 1500 - 1; bad[12].chunk_len = DEBIG_PNG_ENCODE_CHUNK + 1;
        CHECK(emu_png_encode_dynamic_batch(s.data(), slot, row, bad.data(), counts, 13, 2) == 0);
        CHECK(untouched(slot, cap) && untouched(row, 4 * 1500) && untouched(counts, 4));
        std::vector<uint32_t> c(30, 3);
        uint8_t *lens = block(30);
        CTask g = {0, 0, 30, 15};
        std::vector<CTask> cb(6, g);
        cb[0].n = 0; cb[1].n = 287; cb[2].limit = 0; cb[3].limit = 16; cb[4].limit = 4; cb[5].counts_off = 2;
        CHECK(emu_png_encode_codes_batch(c.data(), lens, cb.data(), 6, 0) == 0);
        c[11] = DEBIG_PNG_ENCODE_CODES_MAX_COUNT + 1;
        CHECK(emu_png_encode_codes_batch(c.data(), lens, &g, 1, 0) == 0);
        CHECK(untouched(lens, 30));
        free(slot); free(row); free(counts); free(lens);
    }
    printf("all checks passed\n");
    return 0;
}
