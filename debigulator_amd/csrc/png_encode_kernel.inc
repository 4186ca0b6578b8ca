// png_encode_kernel.inc -- the two kernels behind debig_png_encode_batch (include/decode_png.h, which has the file's rules;
// include/debig_hip.h: debig_hip_png_encode_filter_batch, debig_hip_png_encode_deflate_batch and their tasks).
//
// FILTER   a task is a run of rows of one image for one workgroup of 256 lanes; a wavefront takes a row at a time.  The tensor is
//          read through lbl_load (png_stage_common.inc), HWC or CHW, 16-bit samples go out big-endian, and 1 + row_bytes bytes per
//          row land in the image's filtered stream.  A row reads the RAW row above it, never filtered bytes, so tasks are
//          independent whatever the cut.  ADAPTIVE: S(type) = the sum of min(b, 256 - b) over the row's filtered bytes, the
//          smallest S wins, ties go to the lowest type.  An element that the depth or the palette cannot hold sets the image's
//          flag word with a plain store of 1 (every writer stores the same value).
// DEFLATE  a task is one chunk of at most DEBIG_PNG_ENCODE_CHUNK bytes of an image's filtered stream for ONE WAVEFRONT (a
//          workgroup of 64 lanes).  Its output, in the task's own slot, is a run of complete DEFLATE blocks that starts and ends
//          on a byte boundary: a chunk that is not the image's last ends with an empty stored block, the last one has BFINAL.
//          Level 0: one stored block.  Level 1: one fixed-Huffman block, greedy LZ77, 64 positions per step, one lane each:
//            - a lane hashes its 3 bytes, reads the candidate of a 4096-entry table in LDS and only then inserts itself (the
//              table holds position + 1, inserted by atomicMax: the LATEST position wins by rule, not by store order; the 32 KiB
//              in front of the chunk are inserted first);
//            - it verifies the distances 1 and bpp and the table's candidate against the STREAM (a match never reads at or
//              behind the chunk's end, and never in front of the stream's first byte: every position read from the table is
//              checked against both before it is an address);
//            - every lane walks the step's 64 lengths in LDS the same way (greedy, wave-uniform) and carries "covered until"
//              into the next step;
//            - bit lengths go through a wavefront prefix sum, every token (at most 31 bits) is ORed into at most two words of an
//              LDS buffer, whose complete words go out as dword stores.
//          A level-1 chunk that is not smaller than the same chunk stored is written stored (DEBIG_PNG_ENCODE_NO_STORED in
//          the task's flags switches that off: tests).  The bytes are a pure function of the task and the stream.  No dynamic
//          Huffman blocks, no lazy matching.  No loop waits for another wavefront.
// A task that breaks a bound is skipped (never indexed out of range).  No scratch, no inline assembly.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc and
// png_stage_common.inc in front of it.

#define PEF_THREADS 256u
#define PED_THREADS 64u
#define PED_HASH_BITS 12u
#define PED_WINDOW 32768u
#define PED_MAX_MATCH 258u
#define PED_TOO_FAR 4096u /* a match of 3 bytes further back than this costs about what three literals cost */

// ---- FILTER ----------------------------------------------------------------------------------------------------------------------

DEV_INLINE uint32_t pef_row_bytes(const debig_png_encode_filter_task &t) { return t.w * t.channels * (t.depth >> 3); }

DEV_INLINE bool pef_task_ok(const debig_png_encode_filter_task &t, const void *images, const void *streams, const void *flags)
{
    if (t.dtype > 3u || t.channels == 0u || t.channels > 4u || (t.depth != 8u && t.depth != 16u) || t.layout > 1u || t.filter > 5u)
        return false;
    if ((t.dtype == 0u && t.depth != 8u) || (t.dtype == 1u && t.depth != 16u) || (t.dtype >= 2u && t.channels != 1u)) return false;
    if (t.palette_entries > 256u || (t.palette_entries != 0u && (t.channels != 1u || t.depth != 8u))) return false;
    if (!stage_dim_ok(t.w, t.h) || !stage_rows_ok(t.h, t.row0, t.rows)) return false;
    if (!stage_budget_ok(t.rows, pef_row_bytes(t), DEBIG_PNG_ENCODE_FILTER_BYTES)) return false;
    return stage_addr_ok(images, t.image_off, (1u << t.dtype) - 1u) && stage_addr_ok(streams, t.stream_off, 0u) &&
           stage_addr_ok(flags, 0u, 3u);
}

// byte i of raw row y: the sample's element, its high byte first at depth 16; bad: the element is outside what the file can hold
template <uint32_t ES>
DEV_INLINE uint32_t pef_raw(const uint8_t *img, const debig_png_encode_filter_task &t, uint32_t y, uint32_t i, bool &bad)
{
    const uint32_t s = t.depth == 16u ? i >> 1 : i;
    const uint32_t x = s / t.channels, ch = s - x * t.channels;
    const uint64_t el = t.layout ? ((uint64_t)ch * t.h + y) * t.w + x : ((uint64_t)y * t.w + x) * t.channels + ch;
    const uint2 q = lbl_load<ES>(img + el * ES);
    const uint32_t top = t.palette_entries ? t.palette_entries - 1u : t.depth == 16u ? 65535u : 255u;
    if (q.y != 0u || q.x > top) bad = true;
    if (t.depth == 16u) return (i & 1u) ? q.x & 255u : (q.x >> 8) & 255u;
    return q.x & 255u;
}

DEV_INLINE uint32_t pef_paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int32_t p = (int32_t)a + (int32_t)b - (int32_t)c;
    const int32_t pa = p > (int32_t)a ? p - (int32_t)a : (int32_t)a - p;
    const int32_t pb = p > (int32_t)b ? p - (int32_t)b : (int32_t)b - p;
    const int32_t pc = p > (int32_t)c ? p - (int32_t)c : (int32_t)c - p;
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}

// the filtered byte of type f from the byte x, the one to its left a, the one above b and the one above a
DEV_INLINE uint32_t pef_apply(uint32_t f, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pred = f == 0u ? 0u : f == 1u ? a : f == 2u ? b : f == 3u ? (a + b) >> 1 : pef_paeth(a, b, c);
    return (x - pred) & 255u;
}

DEV_INLINE uint32_t pef_cost(uint32_t v) { return v < 256u - v ? v : 256u - v; }

template <uint32_t ES>
DEV_INLINE void pef_run(const uint8_t *__restrict__ images, uint8_t *__restrict__ streams, uint32_t *__restrict__ flags,
                        const debig_png_encode_filter_task &t, uint32_t tid)
{
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t rb = pef_row_bytes(t), bpp = t.channels * (t.depth >> 3);
    const uint8_t *img = images + t.image_off;
    bool bad = false, other = false;
    for (uint32_t r = wave; r < t.rows; r += PEF_THREADS / 64u) { /* (uniform over the wavefront) */
        const uint32_t y = t.row0 + r;
        uint32_t type = t.filter;
        if (type == 5u) {
            uint32_t s[5] = {0u, 0u, 0u, 0u, 0u};
            for (uint32_t i = lane; i < rb; i += 64u) {
                const uint32_t x = pef_raw<ES>(img, t, y, i, other);
                const uint32_t a = i >= bpp ? pef_raw<ES>(img, t, y, i - bpp, other) : 0u;
                const uint32_t b = y ? pef_raw<ES>(img, t, y - 1u, i, other) : 0u;
                const uint32_t c = (y && i >= bpp) ? pef_raw<ES>(img, t, y - 1u, i - bpp, other) : 0u;
DEV_UNROLL
                for (uint32_t f = 0; f < 5u; f++) s[f] += pef_cost(pef_apply(f, x, a, b, c));
            }
            type = 0u;
            uint32_t best = 0u;
DEV_UNROLL
            for (uint32_t f = 0; f < 5u; f++) {
                uint32_t v = s[f];
DEV_UNROLL
                for (uint32_t d = 32u; d >= 1u; d >>= 1) v += __shfl_xor(v, (int)d);
                if (f == 0u || v < best) {
                    best = v;
                    type = f;
                }
            }
        }
        uint8_t *out = streams + t.stream_off + (uint64_t)y * (1u + rb);
        if (lane == 0u) out[0] = (uint8_t)type;
        for (uint32_t i = lane; i < rb; i += 64u) {
            const uint32_t x = pef_raw<ES>(img, t, y, i, bad);
            const uint32_t a = (type != 0u && type != 2u && i >= bpp) ? pef_raw<ES>(img, t, y, i - bpp, other) : 0u;
            const uint32_t b = (type >= 2u && y) ? pef_raw<ES>(img, t, y - 1u, i, other) : 0u;
            const uint32_t c = (type == 4u && y && i >= bpp) ? pef_raw<ES>(img, t, y - 1u, i - bpp, other) : 0u;
            out[1u + i] = (uint8_t)pef_apply(type, x, a, b, c);
        }
    }
    if (bad) flags[t.flag_idx] = 1u;
}

__global__ void __launch_bounds__(PEF_THREADS)
debig_png_encode_filter_kernel(const uint8_t *__restrict__ images, uint8_t *__restrict__ streams,
                               const debig_png_encode_filter_task *__restrict__ tasks, uint32_t *__restrict__ flags, uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_encode_filter_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!pef_task_ok(t, images, streams, flags)) continue;
        if (t.dtype == 0u) pef_run<1u>(images, streams, flags, t, tid);
        else if (t.dtype == 1u) pef_run<2u>(images, streams, flags, t, tid);
        else if (t.dtype == 2u) pef_run<4u>(images, streams, flags, t, tid);
        else pef_run<8u>(images, streams, flags, t, tid);
    }
}

// ---- DEFLATE ---------------------------------------------------------------------------------------------------------------------

struct PedLds {
    uint32_t hash[1u << PED_HASH_BITS]; /* position + 1 of the latest insert, 0: none */
    uint32_t out[72];                   /* the bits of one step: at most 31 carried in and 64 x 31 */
    uint32_t lens[64];                  /* the match length of each position of the step, 0: a literal */
};

DEV_INLINE bool ped_task_ok(const debig_png_encode_deflate_task &t, const void *streams, const void *slots, const void *counts)
{
    if (t.level > 1u || t.last > 1u || t.bpp == 0u || t.bpp > 8u) return false;
    if (t.chunk_len == 0u || t.chunk_len > DEBIG_PNG_ENCODE_CHUNK) return false;
    if (t.stream_len >= 0xffffffffull || t.chunk_off >= t.stream_len || t.chunk_len > t.stream_len - t.chunk_off) return false;
    if ((uint64_t)t.slot_cap < DEBIG_PNG_ENCODE_SLOT(t.chunk_len)) return false;
    return stage_addr_ok(slots, t.slot_off, 3u) && stage_addr_ok(counts, 0u, 3u) && streams != nullptr;
}

// the n low bits of v, reversed (Huffman codes go out most significant bit first)
DEV_INLINE uint32_t ped_rev(uint32_t v, uint32_t n) { return __brev(v) >> (32u - n); }

DEV_INLINE uint32_t ped_log2(uint32_t v) { return 31u - (uint32_t)__clz(v); } /* v > 0 */

// a literal in the fixed code -> its bits in stream order, n: how many
DEV_INLINE uint64_t ped_literal(uint32_t v, uint32_t &n)
{
    if (v < 144u) {
        n = 8u;
        return ped_rev(0x30u + v, 8u);
    }
    n = 9u;
    return ped_rev(0x190u + (v - 144u), 9u);
}

// a match length 3 .. 258 -> its length symbol - 257 (0 .. 28) | its extra bits << 8 | their value << 16
DEV_INLINE uint32_t ped_len_sym(uint32_t len)
{
    const uint32_t m = len - 3u;
    if (len == 258u) return 28u;
    if (m < 8u) return m;
    const uint32_t eb = ped_log2(m) - 2u;
    return (4u * eb + 4u + ((m >> eb) & 3u)) | (eb << 8) | ((m & ((1u << eb) - 1u)) << 16);
}

// a match distance 1 .. 32768 -> its distance symbol (0 .. 29) | its extra bits << 8 | their value << 16
DEV_INLINE uint32_t ped_dist_sym(uint32_t dist)
{
    const uint32_t dm = dist - 1u;
    if (dm < 4u) return dm;
    const uint32_t eb = ped_log2(dm) - 1u;
    return (2u * eb + 2u + ((dm >> eb) & 1u)) | (eb << 8) | ((dm & ((1u << eb) - 1u)) << 16);
}

// a match (len 3 .. 258, dist 1 .. 32768) in the fixed code -> its bits in stream order, n: how many (at most 31)
DEV_INLINE uint64_t ped_match(uint32_t len, uint32_t dist, uint32_t &n)
{
    const uint32_t ls = ped_len_sym(len), idx = ls & 255u, ds = ped_dist_sym(dist);
    uint32_t ln;
    uint64_t bits;
    if (idx < 23u) { /* symbols 257 .. 279: 7 bits from 0000000 */
        ln = 7u;
        bits = ped_rev(idx + 1u, 7u);
    } else { /* 280 .. 287: 8 bits from 11000000 */
        ln = 8u;
        bits = ped_rev(0xC0u + (idx - 23u), 8u);
    }
    bits |= (uint64_t)(ls >> 16) << ln;
    ln += (ls >> 8) & 255u;
    bits |= (uint64_t)ped_rev(ds & 255u, 5u) << ln;
    ln += 5u;
    bits |= (uint64_t)(ds >> 16) << ln;
    n = ln + ((ds >> 8) & 255u);
    return bits;
}

// how many bytes at a and at b agree, at most maxl
DEV_INLINE uint32_t ped_match_len(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t maxl)
{
    uint32_t l = 0u;
    while (l < maxl && a[l] == b[l]) l++;
    return l;
}

DEV_INLINE uint32_t ped_hash(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return (v * 0x9E3779B1u) >> (32u - PED_HASH_BITS);
}

// the chunk as stored blocks (one: a chunk is shorter than 65536 bytes) -> the bytes written
DEV_INLINE uint32_t ped_stored(const uint8_t *__restrict__ src, uint8_t *__restrict__ slot, uint32_t len, uint32_t last, uint32_t lane)
{
    const uint32_t total = 5u + len + (last ? 0u : 5u);
    uint32_t *ow = reinterpret_cast<uint32_t *>(slot);
    for (uint32_t w = lane; w < (total + 3u) >> 2; w += 64u) {
        uint32_t v = 0u;
DEV_UNROLL
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t j = 4u * w + k;
            uint32_t b = 0u;
            if (j == 0u) b = last;
            else if (j == 1u) b = len & 255u;
            else if (j == 2u) b = len >> 8;
            else if (j == 3u) b = ~len & 255u;
            else if (j == 4u) b = (~len >> 8) & 255u;
            else if (j < 5u + len) b = src[j - 5u];
            else if (j < total) b = j - (5u + len) >= 3u ? 255u : 0u; /* 00 00 00 FF FF */
            v |= b << (8u * k);
        }
        ow[w] = v;
    }
    return total;
}

// the matcher's table before a chunk's first step: empty, then the window in front of the chunk (three bytes from a position may
// reach into the chunk: they are stream bytes)
DEV_INLINE void ped_window(uint32_t *hash, const uint8_t *__restrict__ stream, uint32_t c0, uint64_t stream_len, uint32_t lane)
{
    for (uint32_t k = lane; k < (1u << PED_HASH_BITS); k += 64u) hash[k] = 0u;
    __syncthreads();
    for (uint32_t q = (c0 > PED_WINDOW ? c0 - PED_WINDOW : 0u) + lane; q < c0; q += 64u)
        if ((uint64_t)q + 2u < stream_len) atomicMax(&hash[ped_hash(stream + q)], q + 1u);
    __syncthreads();
}

// one step of the matcher: the 64 positions from `base` of the chunk at c0 -> the lanes whose position starts a token; best, dist:
// this lane's match (best 0: a literal); covered: the first position that no token covers yet, carried from step to step
DEV_INLINE unsigned long long ped_step(uint32_t *hash, uint32_t *lens, const uint8_t *__restrict__ stream, uint32_t c0, uint32_t len, uint32_t bpp,
                                       uint32_t base, uint32_t lane, uint32_t &covered, uint32_t &best_out, uint32_t &dist_out)
{
    const uint32_t p = base + lane, gp = c0 + p;
    const uint32_t maxl = p < len ? (len - p < PED_MAX_MATCH ? len - p : PED_MAX_MATCH) : 0u;
    uint32_t h = 0u, cand = 0u;
    if (maxl >= 3u) {
        h = ped_hash(stream + gp);
        cand = hash[h];
    }
    __syncthreads(); /* every lane has read before any inserts */
    if (maxl >= 3u) atomicMax(&hash[h], gp + 1u);
    uint32_t best = 0u, dist = 0u;
    if (maxl >= 3u && p >= covered) {
        if (gp >= 1u) {
            best = ped_match_len(stream + gp - 1u, stream + gp, maxl);
            dist = 1u;
        }
        if (bpp > 1u && gp >= bpp && best < maxl) {
            const uint32_t l = ped_match_len(stream + gp - bpp, stream + gp, maxl);
            if (l > best) {
                best = l;
                dist = bpp;
            }
        }
        // the table's candidate: a position in front of this one, inside the stream and inside the window
        if (cand != 0u && cand - 1u < gp && gp - (cand - 1u) <= PED_WINDOW && best < maxl) {
            const uint32_t d = gp - (cand - 1u);
            if (d != 1u && d != bpp) {
                const uint32_t l = ped_match_len(stream + gp - d, stream + gp, maxl);
                if (l > best) {
                    best = l;
                    dist = d;
                }
            }
        }
        if (best < 3u || (best == 3u && dist > PED_TOO_FAR)) best = 0u;
    }
    lens[lane] = best;
    __syncthreads();
    // the greedy walk, the same in every lane
    uint32_t q = covered - base; /* covered >= base: a step covers at least its own 64 positions */
    unsigned long long starts = 0ull;
    while (q < 64u && base + q < len) {
        starts |= 1ull << q;
        const uint32_t l = lens[q];
        q += l ? l : 1u;
    }
    covered = base + q;
    best_out = best;
    dist_out = dist;
    return starts;
}

// what ends a block whose last symbol's bits end at obits (`eob` zero bits of it are still to come: the fixed code's end of block is
// 0000000): not the last chunk: an empty stored block (000, padding, 00 00 FF FF); the last: zero padding -> the task's bytes
DEV_INLINE uint32_t ped_trailer(uint32_t *out, uint32_t *ow, uint32_t obits, uint32_t carry, uint32_t eob, uint32_t last, uint32_t lane)
{
    const uint32_t end = obits + eob + (last ? 0u : 3u), end8 = (end + 7u) & ~7u, bytes = (end8 >> 3) + (last ? 0u : 4u);
    const uint32_t w0 = obits >> 5, nw = ((bytes + 3u) >> 2) - w0; /* at most 3 */
    if (lane < 4u) out[lane] = lane == 0u ? carry : 0u;
    __syncthreads();
    if (lane == 0u && !last) {
        const uint32_t off = end8 - (w0 << 5);
        const uint64_t v = (uint64_t)0xFFFF0000u << (off & 31u);
        out[off >> 5] |= (uint32_t)v;
        out[(off >> 5) + 1u] |= (uint32_t)(v >> 32);
    }
    __syncthreads();
    if (lane < nw) ow[w0 + lane] = out[lane];
    __syncthreads();
    return bytes;
}

// the chunk as one fixed-Huffman block -> the bytes written
DEV_INLINE uint32_t ped_fixed(PedLds &L, const uint8_t *__restrict__ stream, uint8_t *__restrict__ slot,
                              const debig_png_encode_deflate_task &t, uint32_t lane)
{
    const uint32_t len = t.chunk_len, c0 = (uint32_t)t.chunk_off;
    uint32_t *ow = reinterpret_cast<uint32_t *>(slot);
    ped_window(L.hash, stream, c0, t.stream_len, lane);
    uint32_t obits = 3u, carry = t.last | 2u, covered = 0u; /* BFINAL, BTYPE 01 */
    for (uint32_t base = 0u; base < len; base += 64u) {
        uint32_t best, dist;
        const unsigned long long starts = ped_step(L.hash, L.lens, stream, c0, len, t.bpp, base, lane, covered, best, dist);
        uint32_t nb = 0u;
        uint64_t bits = 0u;
        if ((starts >> lane) & 1ull) bits = best ? ped_match(best, dist, nb) : ped_literal(stream[c0 + base + lane], nb);
        uint32_t at = nb; /* inclusive prefix sum of the bit counts */
DEV_UNROLL
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t o = __shfl_up(at, d);
            if (lane >= d) at += o;
        }
        const uint32_t step_bits = __shfl(at, 63);
        L.out[lane] = lane == 0u ? carry : 0u;
        if (lane < 8u) L.out[64u + lane] = 0u;
        __syncthreads();
        if (nb) {
            const uint32_t off = (obits & 31u) + at - nb;
            const uint64_t v = bits << (off & 31u);
            atomicOr(&L.out[off >> 5], (uint32_t)v);
            if (v >> 32) atomicOr(&L.out[(off >> 5) + 1u], (uint32_t)(v >> 32));
        }
        __syncthreads();
        const uint32_t total = (obits & 31u) + step_bits, full = total >> 5;
        for (uint32_t k = lane; k < full; k += 64u) ow[(obits >> 5) + k] = L.out[k];
        carry = L.out[full];
        obits += step_bits;
        __syncthreads();
    }
    return ped_trailer(L.out, ow, obits, carry, 7u, t.last, lane);
}

__global__ void __launch_bounds__(PED_THREADS)
debig_png_encode_deflate_kernel(const uint8_t *__restrict__ streams, uint8_t *__restrict__ slots,
                                const debig_png_encode_deflate_task *__restrict__ tasks, uint32_t *__restrict__ counts, uint32_t n_tasks)
{
    __shared__ PedLds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_encode_deflate_task t = tasks[ti];
        // (uniform over the wavefront: every lane skips, or none)
        if (!ped_task_ok(t, streams, slots, counts)) continue;
        const uint8_t *stream = streams + t.stream_off;
        uint8_t *slot = slots + t.slot_off;
        const uint32_t stored = 5u + t.chunk_len + (t.last ? 0u : 5u);
        uint32_t bytes = stored;
        if (t.level == 1u) bytes = ped_fixed(L, stream, slot, t, lane);
        if (t.level == 0u || (bytes >= stored && !(t.flags & DEBIG_PNG_ENCODE_NO_STORED)))
            bytes = ped_stored(stream + t.chunk_off, slot, t.chunk_len, t.last, lane);
        if (lane == 0u) counts[t.count_idx] = bytes;
    }
}
