/* DEVELOPMENT / TEST TOOLING: the checksum kernel (csrc/checksum_kernel.inc) on the CPU lock-step emulator under AddressSanitizer
 * and UBSan, as a stand-alone program (tools/asan_checksum_emu.sh links it with the emulator sources compiled under the same
 * sanitizers -- tools/simt_emu/libdebig_emu_asan.so -- and runs it; no GPU, no Python, nothing preloaded).
 *
 * The kernel reads its spans in aligned 16-byte lines on a grid that starts at the aligned address at or below the span, and byte
 * by byte where a line is only partly inside the span.  Every arena here is a malloc block of exactly the bytes needed: it starts
 * at the 16-byte line of the span's first byte (malloc returns 16-byte aligned blocks; the span starts `front` bytes into it) and
 * ends with the span's last byte.  A load of one byte past the span's last line, or of one byte in front of the aligned floor of
 * its start, is outside the block and ASan's to see; a partial line read as a whole one is, too, wherever the span ends inside it.
 * The spans are the alignment x length grid of tests/checksum_battery.py (every front residue 0 .. 15 x the lengths around a lane
 * load, a 64-byte piece and 1, 2, 3 tiles of 16384 bytes, counted from the span's start and from the grid's) and its ends of the
 * allocation (a block whose last byte sits at every residue: spans from its first byte and spans up to its last).  Both kinds;
 * results against a bytewise CRC-32 and Adler-32 in this file. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <vector>
#include "../include/debig_hip.h"

extern "C" int emu_checksum_batch(const void *arena, const debig_span *spans, uint32_t *out, uint32_t n, uint32_t kind);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
static const int64_t T = 16384;

static uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u, s >> 8; }

static uint32_t crc32_ref(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xffffffffu;
}

static uint32_t adler32_ref(const uint8_t *p, size_t n)
{
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; i++) {
        a = (a + p[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return (b << 16) | a;
}

static unsigned n_spans_run;

/* spans (off, len) of one exactly-sized block: both kinds, results between sentinel words */
static void run_block(const uint8_t *block, const std::vector<debig_span> &spans)
{
    const uint32_t n = (uint32_t)spans.size();
    for (uint32_t kind = 0; kind < 2; kind++) {
        std::vector<uint32_t> out(n + 32, 0xA5A5A5A5u);
        CHECK(emu_checksum_batch(block, spans.data(), out.data() + 16, n, kind) == 0);
        for (uint32_t i = 0; i < 16; i++) CHECK(out[i] == 0xA5A5A5A5u && out[16 + n + i] == 0xA5A5A5A5u);
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t *p = block + spans[i].off;
            const uint32_t want = kind ? adler32_ref(p, spans[i].len) : crc32_ref(p, spans[i].len);
            if (out[16 + i] != want) {
                fprintf(stderr, "kind %u off %llu len %llu: got %08x want %08x\n", kind, (unsigned long long)spans[i].off,
                        (unsigned long long)spans[i].len, out[16 + i], want);
                exit(1);
            }
        }
    }
    n_spans_run += n;
}

/* fill: 0 random, 1 all 0xFF, 2 all zero */
static uint8_t *block_of(size_t n, int fill, uint32_t &seed)
{
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    CHECK(b && ((uintptr_t)b & 15u) == 0);
    for (size_t i = 0; i < n; i++) b[i] = fill == 0 ? (uint8_t)rnd(seed) : fill == 1 ? 0xFF : 0x00;
    return b;
}

int main()
{
    uint32_t seed = 2024;
    unsigned n_grid = 0;
    /* ---- alignment x length: one block per span, front + len bytes, the span at offset front */
    for (int64_t f = 0; f < 16; f++) {
        const int64_t raw[] = {0, 1, 2, 3, 4, 15, 16, 17, 16 - f, 17 - f, 63, 64, 65, 64 - f, 65 - f, T - 1, T, T + 1, T - f - 1, T - f,
                               T - f + 1, 2 * T - f - 1, 2 * T - f, 2 * T - f + 1, 3 * T - f, 3 * T - f + 1};
        std::set<int64_t> lens;
        for (int64_t v : raw) if (v >= 0) lens.insert(v);
        for (int64_t len : lens) {
            for (int fill = 0; fill < 3; fill++) {
                uint8_t *b = block_of((size_t)(f + len), fill, seed);
                run_block(b, {debig_span{(uint64_t)f, (uint64_t)len}});
                free(b);
            }
            n_grid++;
        }
    }
    CHECK(n_grid == 393);
    /* ---- the same spans with span.off = 0 and the arena pointer at residue f: the block's first f bytes lie in front of the arena */
    for (int64_t f = 1; f < 16; f++)
        for (int64_t len : {(int64_t)0, (int64_t)1, 16 - f, 17 - f, (int64_t)17, T - f, T - f + 1, 2 * T - f}) {
            uint8_t *b = block_of((size_t)(f + len), 0, seed);
            run_block(b + f, {debig_span{0, (uint64_t)len}});
            free(b);
        }
    /* ---- the ends of the allocation: the last byte at every residue r; spans from byte 0, spans up to the last byte */
    for (uint64_t r = 0; r < 16; r++) {
        const uint64_t size = (uint64_t)T + 48 + (r + 1) % 16;
        CHECK((size - 1) % 16 == r);
        uint8_t *b = block_of(size, 0, seed);
        std::vector<debig_span> spans = {{0, size}, {0, 1}, {0, 17}};
        for (uint64_t n : {1u, 2u, 15u, 16u, 17u, 33u, 64u, 100u}) spans.push_back(debig_span{size - n, n});
        run_block(b, spans);
        free(b);
    }
    printf("asan_checksum_emu: %u spans x 2 kinds, every result as the bytewise reference\n", n_spans_run);
    return 0;
}
