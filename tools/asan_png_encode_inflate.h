/* DEVELOPMENT / TEST TOOLING: what the stand-alone sanitizer programs of the PNG encode's levels 2 and 3 share
 * (tools/asan_png_encode_dyn_emu.cpp, tools/asan_png_encode_lz_emu.cpp): CHECK, a small inflater of all three block types whose
 * matches may reach into the 32768 bytes in front of the chunk and nowhere else, and heap blocks of exactly their sizes. */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define PAT 0xEE

static uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u, s >> 8; }

struct Bits {
    const uint8_t *d; size_t n, at;
    uint32_t take(uint32_t k) { uint32_t r = 0; for (uint32_t i = 0; i < k; i++, at++) { CHECK(at < 8 * n); r |= (uint32_t)((d[at >> 3] >> (at & 7)) & 1u) << i; } return r; }
};

/* a canonical code from its lengths; sym(): the next symbol of b */
struct Code {
    std::vector<uint8_t> len;
    std::vector<uint32_t> code;
    explicit Code(const std::vector<uint8_t> &l) : len(l), code(l.size(), 0)
    {
        uint32_t bl[17] = {0}, next[17] = {0}, c = 0;
        for (uint8_t v : l) { CHECK(v <= 15); if (v) bl[v]++; }
        for (uint32_t b = 1; b <= 15; b++) { c = (c + bl[b - 1]) << 1; next[b] = c; }
        uint64_t kraft = 0;
        for (size_t s = 0; s < l.size(); s++) if (l[s]) { code[s] = next[l[s]]++; kraft += 1ull << (15 - l[s]); }
        CHECK(kraft == 1ull << 15); /* every code the encoder writes is complete */
    }
    uint32_t sym(Bits &b) const
    {
        uint32_t c = 0;
        for (uint32_t k = 1; k <= 15; k++) {
            c = (c << 1) | b.take(1);
            for (size_t s = 0; s < len.size(); s++) if (len[s] == k && code[s] == c) return (uint32_t)s;
        }
        CHECK(!"a code that the table does not have");
        return 0;
    }
};

/* the blocks in d[0, n): `hist` grows by what they hold -> the type of the first block */
static uint32_t inflate_task(const uint8_t *d, size_t n, std::vector<uint8_t> &hist, bool last)
{
    static const uint16_t lb[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t le[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t db[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                    8193, 12289, 16385, 24577};
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    Bits b = {d, n, 0};
    bool fin = false;
    uint32_t first = 9;
    while (!fin && 8 * n - b.at >= 3) {
        fin = b.take(1);
        const uint32_t bt = b.take(2);
        CHECK(bt <= 2);
        if (first == 9) first = bt;
        if (bt == 0) {
            b.at = (b.at + 7) & ~(size_t)7;
            const uint32_t ln = b.take(16), nl = b.take(16);
            CHECK(ln == (~nl & 0xffffu) && b.at / 8 + ln <= n);
            hist.insert(hist.end(), d + b.at / 8, d + b.at / 8 + ln);
            b.at += 8 * (size_t)ln;
            continue;
        }
        std::vector<uint8_t> ll(288, 8), dl(32, 5); /* the fixed code: 288 and 32 code words */
        if (bt == 1) {
            for (uint32_t s = 144; s < 256; s++) ll[s] = 9;
            for (uint32_t s = 256; s < 280; s++) ll[s] = 7;
        } else {
            const uint32_t hlit = 257 + b.take(5), hdist = 1 + b.take(5), hclen = 4 + b.take(4);
            CHECK(hlit <= 286 && hdist <= 30);
            std::vector<uint8_t> cl(19, 0), lens;
            for (uint32_t i = 0; i < hclen; i++) cl[order[i]] = (uint8_t)b.take(3);
            uint32_t k7 = 0;
            for (uint8_t v : cl) if (v) k7 += 1u << (7 - v);
            CHECK(k7 == 128);
            const Code cc(cl);
            while (lens.size() < hlit + hdist) {
                const uint32_t s = cc.sym(b);
                if (s < 16) lens.push_back((uint8_t)s);
                else if (s == 16) { CHECK(!lens.empty()); lens.insert(lens.end(), 3 + b.take(2), lens.back()); }
                else lens.insert(lens.end(), s == 17 ? 3 + b.take(3) : 11 + b.take(7), 0);
            }
            CHECK(lens.size() == hlit + hdist);
            ll.assign(lens.begin(), lens.begin() + hlit);
            dl.assign(lens.begin() + hlit, lens.end());
        }
        const Code lc(ll), dc(dl);
        for (;;) {
            const uint32_t sym = lc.sym(b);
            if (sym == 256) break;
            if (sym < 256) { hist.push_back((uint8_t)sym); continue; }
            CHECK(sym <= 285);
            const uint32_t len = lb[sym - 257] + b.take(le[sym - 257]), c = dc.sym(b);
            CHECK(c < 30);
            const uint32_t dist = db[c] + b.take(c < 4 ? 0 : c / 2 - 1);
            CHECK(len <= 258 && dist <= 32768 && dist <= hist.size());
            for (uint32_t k = 0; k < len; k++) hist.push_back(hist[hist.size() - dist]);
        }
    }
    CHECK(fin == last && 8 * n - b.at < 8);
    if (!last) CHECK(n >= 4 && d[n - 4] == 0 && d[n - 3] == 0 && d[n - 2] == 0xff && d[n - 1] == 0xff);
    return first;
}

/* a heap block of exactly n bytes, filled with the pattern */
static uint8_t *block(size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    CHECK(p);
    memset(p, PAT, n);
    return p;
}

static bool untouched(const uint8_t *p, size_t n)
{
    for (size_t i = 0; i < n; i++) if (p[i] != PAT) return false;
    return true;
}
