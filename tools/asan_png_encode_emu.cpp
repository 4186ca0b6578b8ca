/* DEVELOPMENT / TEST TOOLING: the two PNG-encode kernels (csrc/png_encode_kernel.inc) on the CPU lock-step emulator under
 * AddressSanitizer and UBSan, as a stand-alone program (tools/asan_png_encode_emu.sh links it with the emulator sources compiled
 * under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * What the kernels READ -- the tensors and the filtered streams -- are heap blocks of exactly their sizes, so a load in front of or
 * behind them (the row above the first row, the bytes left of column 0, a match source in front of the stream, a compare behind
 * the chunk's end at the stream's end) is ASan's to see; what they WRITE lies between guard bytes that must keep their pattern, and
 * a shift or an index outside its range is UBSan's.  The inputs are the seam and edge ones of the pytest battery
 * (tests/test_emu_png_encode.py): 1 x 1 and 1 x N images of every channel count and depth, row bytes around 64 and 256, CHW, wide
 * integers out of range, row runs cut at every seam; stream lengths 1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1, runs of
 * 257 .. 261 equal bytes, the periods of the pixel distances, a run across a chunk seam, a block again at distance 32768 and
 * 32769, bytes >= 144 with the stored fallback switched off, under grids 0, 1 and 3.  The filter output is compared with a plain
 * loop in this file, the deflate output is inflated by a small decoder in this file (stored and fixed-Huffman blocks; a match may
 * reach into the 32768 bytes in front of the chunk and nowhere else).  Tasks that break a bound must leave every block as it is. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/debig_hip.h"

typedef debig_png_encode_filter_task FTask;
typedef debig_png_encode_deflate_task DTask;
extern "C" int emu_png_encode_filter_batch(const void *, void *, const FTask *, void *, uint32_t, uint32_t);
extern "C" int emu_png_encode_deflate_batch(const void *, void *, const DTask *, void *, uint32_t, uint32_t);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define GUARD 64u
#define PAT 0xEE

/* n bytes between two runs of guard bytes, one heap block */
struct Guarded {
    std::vector<uint8_t> b;
    size_t n;
    explicit Guarded(size_t n_) : b(n_ + 2 * GUARD, PAT), n(n_) {}
    uint8_t *p() { return b.data() + GUARD; }
    void check() const
    {
        for (size_t i = 0; i < GUARD; i++) CHECK(b[i] == PAT && b[GUARD + n + i] == PAT);
    }
    bool untouched() const
    {
        for (uint8_t v : b) if (v != PAT) return false;
        return true;
    }
};

static uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u, s >> 8; }

/* ---- the filter kernel ---- */

static int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}

static void filter_case(uint32_t W, uint32_t H, uint32_t Cn, uint32_t dtype, uint32_t depth, uint32_t layout, uint32_t filter, uint32_t rows,
                        uint32_t grid, int spoil_at /* element to put out of range, -1: none */)
{
    const uint32_t es = 1u << dtype, bps = depth / 8u, rb = W * Cn * bps, bpp = Cn * bps, n_el = W * H * Cn;
    uint32_t seed = W * 31u + H * 7u + Cn + depth + filter;
    std::vector<int64_t> v(n_el); /* HWC order */
    for (uint32_t i = 0; i < n_el; i++) v[i] = (i / (Cn * 5u) * 3u + rnd(seed) % 4u) % (1u << depth);
    if (spoil_at >= 0) v[(size_t)spoil_at] = (spoil_at & 1) ? -1 : (int64_t)1 << depth;
    uint8_t *tensor = (uint8_t *)malloc((size_t)n_el * es); /* exactly its size */
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++)
            for (uint32_t c = 0; c < Cn; c++) {
                const size_t el = layout ? ((size_t)c * H + y) * W + x : ((size_t)y * W + x) * Cn + c;
                memcpy(tensor + el * es, &v[((size_t)y * W + x) * Cn + c], es);
            }
    Guarded stream((size_t)H * (1u + rb)), flags(8);
    memset(flags.p(), 0, 8);
    std::vector<FTask> tasks;
    for (uint32_t y0 = 0; y0 < H; y0 += rows) {
        FTask t;
        memset(&t, 0, sizeof t);
        t.w = W; t.h = H; t.row0 = y0; t.rows = H - y0 < rows ? H - y0 : rows;
        t.channels = Cn; t.dtype = dtype; t.depth = depth; t.layout = layout; t.filter = filter; t.flag_idx = 1;
        tasks.push_back(t);
    }
    CHECK(emu_png_encode_filter_batch(tensor, stream.p(), tasks.data(), flags.p(), (uint32_t)tasks.size(), grid) == 0);
    stream.check();
    flags.check();
    uint32_t f[2];
    memcpy(f, flags.p(), 8);
    CHECK(f[0] == 0 && f[1] == (spoil_at >= 0 ? 1u : 0u));
    if (spoil_at < 0) {
        std::vector<int> raw((size_t)H * rb);
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t i = 0; i < rb; i++) {
                const int64_t s = v[(size_t)y * W * Cn + i / bps];
                raw[(size_t)y * rb + i] = bps == 2 ? (int)((i & 1u) ? s & 255 : s >> 8) : (int)s;
            }
        for (uint32_t y = 0; y < H; y++) {
            const uint8_t *got = stream.p() + (size_t)y * (1u + rb);
            long best = -1;
            uint32_t type = 0;
            std::vector<uint8_t> rowf[5];
            for (uint32_t ft = 0; ft < 5; ft++) {
                long cost = 0;
                for (uint32_t i = 0; i < rb; i++) {
                    const int x = raw[(size_t)y * rb + i], a = i >= bpp ? raw[(size_t)y * rb + i - bpp] : 0, b = y ? raw[(size_t)(y - 1) * rb + i] : 0,
                              c = (y && i >= bpp) ? raw[(size_t)(y - 1) * rb + i - bpp] : 0;
                    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) / 2 : paeth(a, b, c);
                    const uint8_t o = (uint8_t)(x - pred);
                    rowf[ft].push_back(o);
                    cost += o < 256 - o ? o : 256 - o;
                }
                if (best < 0 || cost < best) { best = cost; type = ft; }
            }
            if (filter < 5) type = filter;
            CHECK(got[0] == type);
            CHECK(rb == 0 || memcmp(got + 1, rowf[type].data(), rb) == 0);
        }
    }
    free(tensor);
}

/* ---- the deflate kernel ---- */

struct Bits {
    const uint8_t *d; size_t n, at;
    uint32_t take(uint32_t k) { uint32_t r = 0; for (uint32_t i = 0; i < k; i++, at++) { CHECK(at < 8 * n); r |= (uint32_t)((d[at >> 3] >> (at & 7)) & 1u) << i; } return r; }
    uint32_t code(uint32_t k) { uint32_t r = 0; for (uint32_t i = 0; i < k; i++) r = (r << 1) | take(1); return r; }
};

/* the blocks in d[0, n): `hist` (the stream up to the chunk) grows by what they hold; a match reaches at most 32768 bytes back and
 * never in front of the stream -> whether the last block had BFINAL */
static bool inflate_task(const uint8_t *d, size_t n, std::vector<uint8_t> &hist, bool last)
{
    static const uint16_t lb[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t le[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t db[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                    8193, 12289, 16385, 24577};
    Bits b = {d, n, 0};
    bool fin = false;
    while (!fin && 8 * n - b.at >= 3) {
        fin = b.take(1);
        const uint32_t bt = b.take(2);
        CHECK(bt <= 1);
        if (bt == 0) {
            b.at = (b.at + 7) & ~(size_t)7;
            const uint32_t ln = b.take(16), nl = b.take(16);
            CHECK(ln == (~nl & 0xffffu) && b.at / 8 + ln <= n);
            hist.insert(hist.end(), d + b.at / 8, d + b.at / 8 + ln);
            b.at += 8 * (size_t)ln;
            continue;
        }
        for (;;) {
            uint32_t c = b.code(7), sym;
            if (c <= 23) sym = 256 + c;
            else {
                c = (c << 1) | b.take(1);
                if (c >= 0x30 && c <= 0xBF) sym = c - 0x30;
                else if (c >= 0xC0 && c <= 0xC7) sym = 280 + c - 0xC0;
                else { c = (c << 1) | b.take(1); CHECK(c >= 0x190); sym = 144 + c - 0x190; }
            }
            if (sym == 256) break;
            if (sym < 256) { hist.push_back((uint8_t)sym); continue; }
            CHECK(sym <= 285);
            const uint32_t len = lb[sym - 257] + b.take(le[sym - 257]), dc = b.code(5);
            CHECK(dc < 30);
            const uint32_t dist = db[dc] + b.take(dc < 4 ? 0 : dc / 2 - 1);
            CHECK(len <= 258 && dist <= 32768 && dist <= hist.size());
            for (uint32_t k = 0; k < len; k++) hist.push_back(hist[hist.size() - dist]);
        }
    }
    CHECK(fin == last && 8 * n - b.at < 8);
    if (!last) CHECK(n >= 4 && d[n - 4] == 0 && d[n - 3] == 0 && d[n - 2] == 0xff && d[n - 1] == 0xff);
    return fin;
}

static void deflate_case(const std::vector<uint8_t> &s, uint32_t level, uint32_t bpp, uint32_t flags)
{
    const uint32_t C = DEBIG_PNG_ENCODE_CHUNK, nt = (uint32_t)((s.size() + C - 1) / C);
    uint8_t *stream = (uint8_t *)malloc(s.size()); /* exactly its size */
    memcpy(stream, s.data(), s.size());
    std::vector<std::vector<uint8_t>> first;
    for (uint32_t grid : {0u, 1u, 3u}) {
        std::vector<Guarded> slots;
        std::vector<DTask> tasks(nt);
        size_t total = 0;
        for (uint32_t k = 0; k < nt; k++) total += (size_t)DEBIG_PNG_ENCODE_SLOT(k + 1 == nt ? s.size() - (size_t)k * C : C) + 2 * GUARD;
        Guarded all(total), counts(4 * (size_t)nt);
        size_t at = GUARD; /* every slot between guard bytes of its own */
        for (uint32_t k = 0; k < nt; k++) {
            DTask &t = tasks[grid == 1 ? nt - 1 - k : k]; /* grid 1: the tasks in reversed order */
            memset(&t, 0, sizeof t);
            t.stream_len = s.size(); t.chunk_off = (uint64_t)k * C;
            t.chunk_len = (uint32_t)(k + 1 == nt ? s.size() - (size_t)k * C : C);
            t.slot_cap = (uint32_t)DEBIG_PNG_ENCODE_SLOT(t.chunk_len); t.slot_off = at;
            t.level = level; t.bpp = bpp; t.last = k + 1 == nt; t.count_idx = k; t.flags = flags;
            at += t.slot_cap + 2 * GUARD;
        }
        CHECK(emu_png_encode_deflate_batch(stream, all.p(), tasks.data(), counts.p(), nt, grid) == 0);
        all.check();
        counts.check();
        std::vector<uint8_t> hist;
        for (uint32_t k = 0; k < nt; k++) {
            const DTask &t = tasks[grid == 1 ? nt - 1 - k : k];
            uint32_t n;
            memcpy(&n, counts.p() + 4 * (size_t)k, 4);
            CHECK(n > 0 && n <= t.slot_cap);
            const uint8_t *o = all.p() + t.slot_off;
            for (uint32_t g = 0; g < GUARD; g++) CHECK(o[-(int)g - 1] == PAT && o[t.slot_cap + g] == PAT);
            const uint32_t stored = 5u + t.chunk_len + (t.last ? 0u : 5u);
            if (level == 0) CHECK(n == stored);
            else if (!flags) CHECK(n <= stored);
            /* the window: only the 32768 bytes in front of the chunk may be referenced */
            std::vector<uint8_t> win(hist.end() - (hist.size() < 32768 ? hist.size() : 32768), hist.end());
            const size_t before = win.size();
            inflate_task(o, n, win, t.last != 0);
            CHECK(win.size() - before == t.chunk_len && memcmp(win.data() + before, s.data() + t.chunk_off, t.chunk_len) == 0);
            hist.insert(hist.end(), win.begin() + before, win.end());
            std::vector<uint8_t> bytes(o, o + n);
            if (grid == 0) first.push_back(bytes);
            else CHECK(first[k] == bytes); /* the same bytes for every grid and order */
        }
        CHECK(hist == s);
    }
    free(stream);
}

static std::vector<uint8_t> noise(size_t n, uint32_t seed, uint32_t lo, uint32_t span)
{
    std::vector<uint8_t> v(n);
    for (auto &b : v) b = (uint8_t)(lo + rnd(seed) % span);
    return v;
}

int main()
{
    /* the filter kernel */
    for (uint32_t Cn = 1; Cn <= 4; Cn++)
        for (uint32_t dtype = 0; dtype < 2; dtype++)
            for (uint32_t filter = 0; filter < 6; filter++) {
                filter_case(1, 1, Cn, dtype, dtype ? 16 : 8, 0, filter, 1, 0, -1);
                filter_case(7, 1, Cn, dtype, dtype ? 16 : 8, 1, filter, 1, 0, -1);
                filter_case(5, 3, Cn, dtype, dtype ? 16 : 8, Cn & 1, filter, 2, 1, -1);
            }
    for (uint32_t rb : {63u, 64u, 65u, 255u, 256u, 257u})
        for (uint32_t filter : {4u, 5u}) filter_case(rb, 4, 1, 0, 8, 0, filter, 3, 2, -1);
    for (uint32_t rows = 1; rows <= 5; rows++) filter_case(21, 5, 3, 0, 8, 1, 5, rows, 2, -1);
    for (uint32_t dtype = 2; dtype < 4; dtype++)
        for (uint32_t depth : {8u, 16u}) {
            filter_case(13, 7, 1, dtype, depth, 0, 5, 4, 0, -1);
            for (int at : {0, 44, 13 * 7 - 1}) filter_case(13, 7, 1, dtype, depth, 0, 5, 4, 0, at);
        }
    /* the deflate kernel */
    const uint32_t C = DEBIG_PNG_ENCODE_CHUNK;
    for (uint32_t level = 0; level < 2; level++)
        for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)C - 1, (size_t)C, (size_t)C + 1, (size_t)2 * C + 1}) {
            std::vector<uint8_t> s = noise(n, (uint32_t)n, 0, 40);
            for (size_t i = 0; i + 2 < n; i += 3) s[i + 1] = s[i + 2] = s[i]; /* triples: short matches everywhere */
            deflate_case(s, level, 3, 0);
        }
    for (uint32_t n = 1; n <= 8; n++) deflate_case(noise(n, n, 144, 112), 1, 1, DEBIG_PNG_ENCODE_NO_STORED);
    deflate_case({0, 143, 144, 255, 143, 0, 255, 144}, 1, 1, DEBIG_PNG_ENCODE_NO_STORED);
    for (uint32_t n = 257; n <= 262; n++) {
        std::vector<uint8_t> s(n + 1, 200);
        s[0] = 7;
        deflate_case(s, 1, 1, 0);
    }
    for (uint32_t period : {2u, 3u, 4u, 6u, 8u}) {
        std::vector<uint8_t> unit = noise(period, period, 0, 256), s;
        for (uint32_t i = 0; i < 1500; i++) s.push_back(unit[i % period]);
        deflate_case(s, 1, period, 0);
        deflate_case(s, 1, 1, 0);
    }
    {
        std::vector<uint8_t> s = noise(C - 100, 1, 0, 256);
        s.insert(s.end(), 400, 9);
        s.insert(s.end(), s.begin(), s.begin() + 50);
        deflate_case(s, 1, 1, 0);
    }
    for (uint32_t period : {32768u, 32769u}) {
        std::vector<uint8_t> block = noise(300, period, 0, 256), s = block;
        s.resize(period, 0);
        s.insert(s.end(), block.begin(), block.end());
        s.push_back('e');
        deflate_case(s, 1, 1, 0);
        std::vector<uint8_t> big = noise(period, period + 1, 0, 256), twice = big;
        twice.insert(twice.end(), big.begin(), big.end());
        deflate_case(twice, 1, 4, 0);
    }
    deflate_case({'a', 'b', 'c', 'X', 'Y', 'Z', 'a', 'b', 'c', 'a', 'b', 'c', 0, 0, 0, 0}, 1, 8, 0);
    deflate_case(std::vector<uint8_t>(2 * C + 77, 0), 1, 1, 0);
    deflate_case(noise(C + 500, 2, 144, 112), 1, 1, 0);
    /* tasks that break a bound leave every block as it is */
    {
        std::vector<uint8_t> s = noise(1500, 4, 0, 9);
        Guarded slot((size_t)DEBIG_PNG_ENCODE_SLOT(1500)), counts(4);
        DTask good;
        memset(&good, 0, sizeof good);
        good.stream_len = 1500; good.chunk_len = 1500; good.slot_cap = (uint32_t)DEBIG_PNG_ENCODE_SLOT(1500); good.level = 1; good.bpp = 1; good.last = 1;
        std::vector<DTask> bad(9, good);
        bad[0].chunk_len = 0; bad[1].chunk_off = 1500; bad[2].chunk_len = 1501; bad[3].slot_cap -= 16; bad[4].level = 2; bad[5].last = 2;
        bad[6].bpp = 0; bad[7].bpp = 9; bad[8].slot_off = 2;
        CHECK(emu_png_encode_deflate_batch(s.data(), slot.p(), bad.data(), counts.p(), 9, 2) == 0);
        CHECK(slot.untouched() && counts.untouched());
        Guarded stream(6 * 11), flags(4);
        std::vector<uint8_t> tensor(6 * 10, 1);
        FTask fg;
        memset(&fg, 0, sizeof fg);
        fg.w = 10; fg.h = 6; fg.rows = 6; fg.channels = 1; fg.depth = 8; fg.filter = 5;
        std::vector<FTask> fb(10, fg);
        fb[0].w = 0; fb[1].h = 16385; fb[2].rows = 0; fb[3].row0 = 6; fb[4].rows = 7; fb[5].channels = 5; fb[6].dtype = 4; fb[7].depth = 12;
        fb[8].filter = 6; fb[9].palette_entries = 257;
        CHECK(emu_png_encode_filter_batch(tensor.data(), stream.p(), fb.data(), flags.p(), 10, 3) == 0);
        CHECK(stream.untouched() && flags.untouched());
    }
    printf("all checks passed\n");
    return 0;
}
