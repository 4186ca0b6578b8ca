// png_encode_dynamic_kernel.inc -- level 2 of the PNG encode (include/decode_png.h: debig_png_encode_batch_dyn; include/debig_hip.h
// has the rules of the format word for word: debig_hip_png_encode_dynamic_batch, debig_hip_png_encode_codes_batch and their tasks).
//
// DYNAMIC  one wavefront per chunk task, four phases:
//   MATCH   level 1's step (ped_window, ped_step of png_encode_kernel.inc: the matcher exists once).  A lane whose position starts a
//           token stores it -- 32 bits: a literal's byte, or bit 31, length - 3 in bits 16 .. 23 and distance - 1 in bits 0 .. 14 --
//           at the running count plus the number of starting lanes below it, and adds into the literal/length and the distance
//           histogram in LDS.
//   BUILD   pdy_lengths for the two alphabets, the header's run-length coding (one lane: at most 316 lengths), pdy_lengths for the
//           code-length alphabet, pdy_codes for all three.
//   CHOICE  the exact bits of the chunk in the fixed and in the dynamic code, from the histograms, and the stored bytes.
//   EMIT    the chosen block: 64 header symbols, then 64 tokens of the row per step, codes from a table in LDS, offsets from the
//           wavefront prefix sum; a token of up to 48 bits is ORed into at most three words of the step buffer.  The end of block is
//           the row's last token; the trailer is ped_trailer.  Fixed and stored blocks are level 1's bytes: the same tokens in the
//           same code.
// pdy_lengths splits the rule's work like this: every lane ranks its symbols by counting the used symbols in front of them; ONE
// lane runs the at most 285 merge steps of the two queues and the depths of the internal nodes; every lane takes its leaves'
// depths; one lane runs the limiter on num[]; every lane hands its ranks their lengths.  None of it changes the result.
// CODES    a task is one call of pdy_lengths: the battery's way to the builder.
// Every index that was read from LDS or from the token row is masked or compared before it is an address.  No loop waits for another
// wavefront.  No scratch, no inline assembly.  A task that breaks a bound is skipped.
// Included behind png_encode_kernel.inc by debig_hip.hip (hipcc) and by the CPU emulator build (tests).

#define PDY_LL 288u  /* cnt, tab, len8: the literal/length alphabet from 0 (286 symbols) ... */
#define PDY_D 32u    /* ... the distance alphabet from PDY_LL (30) ...                        */
#define PDY_CL 32u   /* ... the code-length alphabet from PDY_LL + PDY_D (19)                 */
#define PDY_SYMS (PDY_LL + PDY_D + PDY_CL)
#define PDY_HDR 320u /* at most 286 + 30 header symbols */
#define PDY_OUT 104u /* the bits of one step: at most 31 carried in and 64 x 48, and the two words a token may spill into */
#define PDY_EOB 0x40000000u

struct PdyBuild {
    uint32_t w[PDY_LL];        /* the used symbols' counts in the rule's order                */
    uint32_t iw[PDY_LL];       /* the internal nodes' weights in creation order               */
    uint16_t order[PDY_LL];    /* rank -> symbol                                              */
    uint16_t lparent[PDY_LL];  /* rank -> the internal node above the leaf                    */
    uint16_t iparent[PDY_LL];  /* internal node -> the one above it                           */
    uint16_t idepth[PDY_LL];   /* internal node -> its depth                                  */
    uint32_t num[16];          /* the leaves of each depth; pdy_codes: the symbols of a length */
    uint32_t next[16];         /* pdy_codes: the first code of each length                    */
};

struct PdyLate { /* what only BUILD and EMIT need */
    uint32_t out[PDY_OUT];
    uint32_t tab[PDY_SYMS]; /* the code in stream order | its length << 16 */
    uint16_t hdr[PDY_HDR];  /* a header symbol | the value of its extra bits << 8 */
    PdyBuild B;
};

struct PdyLds {
    union {
        uint32_t hash[1u << PED_HASH_BITS]; /* MATCH: the matcher's table ... */
        PdyLate late;                       /* ... whose 16 KiB are free behind it: 18.0 KiB per wavefront, eight wavefronts per CU */
    } u;
    uint32_t lens[64];
    uint32_t cnt[PDY_SYMS];
    uint8_t len8[PDY_SYMS];
    uint32_t misc[4]; /* HLIT, HDIST, HCLEN, the header symbols */
};

struct PdyCodesLds {
    uint32_t cnt[PDY_LL];
    uint8_t len8[PDY_LL];
    PdyBuild B;
};

DEV_INLINE uint32_t pdy_sum(uint32_t v)
{
DEV_UNROLL
    for (uint32_t d = 32u; d >= 1u; d >>= 1) v += __shfl_xor(v, (int)d);
    return v;
}

// the rule of include/debig_hip.h: cnt[0, n) -> len[0, n), every length 0 .. limit.  n 1 .. 286, limit 1 .. 15, 1 << limit >= n, the
// counts' sum fits 32 bits.  (uniform over the wavefront: every lane calls it with the same arguments)
DEV_INLINE void pdy_lengths(const uint32_t *cnt, uint32_t n, uint32_t limit, uint8_t *len, PdyBuild &B, uint32_t lane)
{
    uint32_t nu = 0u;
    for (uint32_t s = lane; s < n; s += 64u) {
        len[s] = 0u;
        if (cnt[s]) nu++;
    }
    nu = pdy_sum(nu);
    if (lane < 16u) B.num[lane] = 0u;
    __syncthreads();
    if (nu < 2u) { /* (uniform) */
        if (lane == 0u) {
            uint32_t k = 0u;
            for (uint32_t s = 0u; s < n; s++)
                if (cnt[s]) {
                    len[s] = 1u;
                    k++;
                }
            for (uint32_t s = 0u; s < n && k < 2u; s++)
                if (!cnt[s]) {
                    len[s] = 1u;
                    k++;
                }
        }
        __syncthreads();
        return;
    }
    // the order: a symbol's rank is the number of used symbols with a smaller (count, index)
    for (uint32_t s = lane; s < n; s += 64u) {
        const uint32_t c = cnt[s];
        if (!c) continue;
        uint32_t r = 0u;
        for (uint32_t t = 0u; t < n; t++) {
            const uint32_t ct = cnt[t];
            if (ct && (ct < c || (ct == c && t < s))) r++;
        }
        B.order[r] = (uint16_t)s; /* r < nu <= n */
        B.w[r] = c;
    }
    __syncthreads();
    if (lane == 0u) {
        // the two queues: li the front leaf, ii the front internal node, ni the internal nodes made; nu - 1 steps, each takes two
        uint32_t li = 0u, ii = 0u, ni = 0u;
        for (uint32_t k = 0u; k + 1u < nu; k++) {
            uint32_t sum = 0u;
            for (uint32_t pick = 0u; pick < 2u; pick++) {
                if (li < nu && (ii >= ni || B.w[li] <= B.iw[ii])) { /* a tie: the leaf */
                    sum += B.w[li];
                    B.lparent[li++] = (uint16_t)ni;
                } else {
                    sum += B.iw[ii];
                    B.iparent[ii++] = (uint16_t)ni;
                }
            }
            B.iw[ni++] = sum;
        }
        // a node is made behind everything below it: the depths from the root down
        B.idepth[nu - 2u] = 0u;
        for (uint32_t j = nu - 2u; j-- > 0u;) {
            const uint32_t p = B.iparent[j];
            B.idepth[j] = (uint16_t)((p < PDY_LL ? B.idepth[p] : 0u) + 1u);
        }
    }
    __syncthreads();
    for (uint32_t r = lane; r < nu; r += 64u) {
        const uint32_t p = B.lparent[r];
        uint32_t d = (p < PDY_LL ? B.idepth[p] : 0u) + 1u;
        if (d > limit) d = limit;
        atomicAdd(&B.num[d], 1u);
    }
    __syncthreads();
    if (lane == 0u) {
        uint32_t total = 0u;
        for (uint32_t l = 1u; l <= limit; l++) total += B.num[l] << (limit - l);
        while (total > (1u << limit) && B.num[limit]) {
            uint32_t l = limit - 1u;
            while (l && !B.num[l]) l--;
            if (!l) break; /* (never: 1 << limit >= n) */
            B.num[limit] -= 1u;
            B.num[l] -= 1u;
            B.num[l + 1u] += 2u;
            total--;
        }
    }
    __syncthreads();
    for (uint32_t r = lane; r < nu; r += 64u) {
        uint32_t l = limit, acc = B.num[limit];
        while (l > 1u && r >= acc) acc += B.num[--l];
        const uint32_t s = B.order[r];
        if (s < n) len[s] = (uint8_t)l;
    }
    __syncthreads();
}

// canonical codes (RFC 1951 3.2.2) of len[0, n) -> tab[0, n): the code in stream order | its length << 16, 0 for an unused symbol
DEV_INLINE void pdy_codes(const uint8_t *len, uint32_t n, uint32_t *tab, PdyBuild &B, uint32_t lane)
{
    if (lane < 16u) B.num[lane] = 0u;
    __syncthreads();
    for (uint32_t s = lane; s < n; s += 64u) {
        const uint32_t l = len[s] & 15u;
        if (l) atomicAdd(&B.num[l], 1u);
    }
    __syncthreads();
    if (lane == 0u) {
        uint32_t code = 0u;
        B.next[0] = 0u;
        for (uint32_t l = 1u; l < 16u; l++) {
            code = (code + (l > 1u ? B.num[l - 1u] : 0u)) << 1;
            B.next[l] = code;
        }
    }
    __syncthreads();
    for (uint32_t s = lane; s < n; s += 64u) {
        const uint32_t l = len[s] & 15u;
        uint32_t e = 0u;
        if (l) {
            uint32_t k = 0u;
            for (uint32_t t = 0u; t < s; t++) k += (len[t] & 15u) == l;
            e = ped_rev((B.next[l] + k) & ((1u << l) - 1u), l) | (l << 16);
        }
        tab[s] = e;
    }
    __syncthreads();
}

// the extra bits of literal/length symbol s, of distance symbol d, of code-length symbol c; the fixed code's length of s
DEV_INLINE uint32_t pdy_lext(uint32_t s) { return (s < 265u || s >= 285u) ? 0u : (s - 261u) >> 2; }
DEV_INLINE uint32_t pdy_dext(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }
DEV_INLINE uint32_t pdy_cext(uint32_t c) { return c == 16u ? 2u : c == 17u ? 3u : c == 18u ? 7u : 0u; }
DEV_INLINE uint32_t pdy_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
// the RFC's order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
DEV_INLINE uint32_t pdy_cl_order(uint32_t i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12u ? lo >> (5u * i) : hi >> (5u * (i < 19u ? i - 12u : 6u))) & 31u);
}

// the header's symbols from the two length lists (one lane): L.u.late.hdr, their counts in L.cnt, HLIT, HDIST and their number in L.misc
DEV_INLINE void pdy_header(PdyLds &L)
{
    uint32_t hlit = 286u, hdist = 30u, nh = 0u;
    while (hlit > 257u && !L.len8[hlit - 1u]) hlit--;
    while (hdist > 1u && !L.len8[PDY_LL + hdist - 1u]) hdist--;
    const uint32_t total = hlit + hdist;
    for (uint32_t i = 0u; i < total;) {
        const uint32_t v = L.len8[i < hlit ? i : PDY_LL + (i - hlit)] & 15u;
        uint32_t run = 1u;
        while (i + run < total && (L.len8[i + run < hlit ? i + run : PDY_LL + (i + run - hlit)] & 15u) == v) run++;
        i += run;
        while (run) {
            uint32_t sym = v, ex = 0u, take = 1u;
            if (v == 0u && run >= 11u) {
                take = run < 138u ? run : 138u;
                sym = 18u;
                ex = take - 11u;
            } else if (v == 0u && run >= 3u) {
                take = run;
                sym = 17u;
                ex = take - 3u;
            }
            if (nh < PDY_HDR) L.u.late.hdr[nh] = (uint16_t)(sym | (ex << 8));
            nh++;
            L.cnt[PDY_LL + PDY_D + sym] += 1u;
            run -= take;
            if (v != 0u)
                while (run >= 3u) { /* the value once, then its repeats */
                    take = run < 6u ? run : 6u;
                    if (nh < PDY_HDR) L.u.late.hdr[nh] = (uint16_t)(16u | ((take - 3u) << 8));
                    nh++;
                    L.cnt[PDY_LL + PDY_D + 16u] += 1u;
                    run -= take;
                }
        }
    }
    L.misc[0] = hlit;
    L.misc[1] = hdist;
    L.misc[3] = nh < PDY_HDR ? nh : PDY_HDR;
}

// a token of the row in the fixed (dyn false) or in the dynamic code -> its bits in stream order, nb: how many (at most 48)
DEV_INLINE uint64_t pdy_token(const PdyLds &L, uint32_t tok, bool dyn, uint32_t &nb)
{
    if (!(tok >> 31)) {
        const uint32_t s = (tok & PDY_EOB) ? 256u : tok & 255u;
        if (!dyn) {
            if (s == 256u) {
                nb = 7u;
                return 0u;
            }
            return ped_literal(s, nb);
        }
        const uint32_t e = L.u.late.tab[s];
        nb = e >> 16;
        return e & 0xffffu;
    }
    const uint32_t len = 3u + ((tok >> 16) & 255u), dist = 1u + (tok & 0x7fffu);
    if (!dyn) return ped_match(len, dist, nb);
    const uint32_t ls = ped_len_sym(len), ds = ped_dist_sym(dist);
    uint32_t e = L.u.late.tab[257u + (ls & 255u)];
    uint64_t bits = e & 0xffffu;
    uint32_t n = e >> 16;
    bits |= (uint64_t)(ls >> 16) << n;
    n += (ls >> 8) & 255u;
    e = L.u.late.tab[PDY_LL + (ds & 255u)];
    bits |= (uint64_t)(e & 0xffffu) << n;
    n += e >> 16;
    bits |= (uint64_t)(ds >> 16) << n;
    nb = n + ((ds >> 8) & 255u);
    return bits;
}

// one step of the emit: every lane's nb bits (at most 48; 0: none) behind the obits bits written so far, in lane order
DEV_INLINE void pdy_put(uint32_t *out, uint32_t *ow, uint32_t &obits, uint32_t &carry, uint64_t bits, uint32_t nb, uint32_t lane)
{
    uint32_t at = nb; /* inclusive prefix sum of the bit counts */
DEV_UNROLL
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(at, d);
        if (lane >= d) at += o;
    }
    const uint32_t step_bits = __shfl(at, 63);
    out[lane] = lane == 0u ? carry : 0u;
    if (lane < PDY_OUT - 64u) out[64u + lane] = 0u;
    __syncthreads();
    if (nb) {
        const uint32_t off = (obits & 31u) + at - nb, sh = off & 31u, w = off >> 5; /* w + 2 <= (31 + 64 x 48) / 32 + 2 < PDY_OUT */
        const uint64_t rest = bits >> (32u - sh);
        atomicOr(&out[w], (uint32_t)(bits << sh));
        if ((uint32_t)rest) atomicOr(&out[w + 1u], (uint32_t)rest);
        if (rest >> 32) atomicOr(&out[w + 2u], (uint32_t)(rest >> 32));
    }
    __syncthreads();
    const uint32_t total = (obits & 31u) + step_bits, full = total >> 5;
    for (uint32_t k = lane; k < full; k += 64u) ow[(obits >> 5) + k] = out[k];
    carry = out[full];
    obits += step_bits;
    __syncthreads();
}

DEV_INLINE bool pdy_task_ok(const debig_png_encode_dynamic_task &t, const void *streams, const void *slots, const void *tokens, const void *counts)
{
    if (t.level != 2u || t.last > 1u || t.bpp == 0u || t.bpp > 8u) return false;
    if (t.chunk_len == 0u || t.chunk_len > DEBIG_PNG_ENCODE_CHUNK) return false;
    if (t.stream_len >= 0xffffffffull || t.chunk_off >= t.stream_len || t.chunk_len > t.stream_len - t.chunk_off) return false;
    if ((uint64_t)t.slot_cap < DEBIG_PNG_ENCODE_SLOT(t.chunk_len) || t.token_cap / 4u < t.chunk_len) return false;
    return stage_addr_ok(slots, t.slot_off, 3u) && stage_addr_ok(tokens, t.token_off, 3u) && stage_addr_ok(counts, 0u, 3u) && streams != nullptr;
}

// MATCH, the end of a step: a lane whose position starts a token (best 0: the literal at `at`) stores it behind the ntok tokens of the
// steps before and counts its symbols
DEV_INLINE void pdy_step_tokens(PdyLds &L, uint32_t *row, uint32_t token_cap, unsigned long long starts, uint32_t &ntok, uint32_t best,
                                uint32_t dist, const uint8_t *__restrict__ at, uint32_t lane)
{
    if ((starts >> lane) & 1ull) {
        const uint32_t idx = ntok + (uint32_t)__popcll(starts & ((1ull << lane) - 1ull));
        uint32_t tok;
        if (best) {
            tok = 0x80000000u | ((best - 3u) << 16) | (dist - 1u);
            atomicAdd(&L.cnt[257u + (ped_len_sym(best) & 255u)], 1u);
            atomicAdd(&L.cnt[PDY_LL + (ped_dist_sym(dist) & 255u)], 1u);
        } else {
            tok = *at;
            atomicAdd(&L.cnt[tok], 1u);
        }
        if (idx < token_cap / 4u) row[idx] = tok; /* (always: a chunk has at most chunk_len tokens) */
    }
    ntok += (uint32_t)__popcll(starts);
}

// MATCH of level 2 -> the tokens in the row
DEV_INLINE uint32_t pdy_match(PdyLds &L, const uint8_t *__restrict__ stream, uint32_t *row, const debig_png_encode_dynamic_task &t, uint32_t lane)
{
    const uint32_t len = t.chunk_len, c0 = (uint32_t)t.chunk_off;
    for (uint32_t k = lane; k < PDY_SYMS; k += 64u) L.cnt[k] = 0u;
    ped_window(L.u.hash, stream, c0, t.stream_len, lane);
    uint32_t covered = 0u, ntok = 0u;
    for (uint32_t base = 0u; base < len; base += 64u) {
        uint32_t best, dist;
        const unsigned long long starts = ped_step(L.u.hash, L.lens, stream, c0, len, t.bpp, base, lane, covered, best, dist);
        pdy_step_tokens(L, row, t.token_cap, starts, ntok, best, dist, stream + c0 + base + lane, lane);
    }
    return ntok;
}

// BUILD, CHOICE and EMIT: the block of the ntok tokens that MATCH left in the row and in the histograms -> the bytes written.  T: the
// dynamic task, or the level-3 task (png_encode_lz_kernel.inc), which has the same fields in the same places
template <class T>
DEV_INLINE uint32_t pdy_finish(PdyLds &L, const uint8_t *__restrict__ stream, uint8_t *__restrict__ slot, const uint32_t *row, const T &t,
                               uint32_t ntok, uint32_t lane)
{
    const uint32_t len = t.chunk_len, c0 = (uint32_t)t.chunk_off;
    uint32_t *ow = reinterpret_cast<uint32_t *>(slot);
    if (ntok > t.token_cap / 4u) ntok = t.token_cap / 4u;
    if (lane == 0u) L.cnt[256] = 1u; /* the end of block */
    __syncthreads();
    // ---- BUILD ----
    pdy_lengths(L.cnt, 286u, 15u, L.len8, L.u.late.B, lane);
    pdy_lengths(L.cnt + PDY_LL, 30u, 15u, L.len8 + PDY_LL, L.u.late.B, lane);
    if (lane == 0u) pdy_header(L);
    __syncthreads();
    pdy_lengths(L.cnt + PDY_LL + PDY_D, 19u, 7u, L.len8 + PDY_LL + PDY_D, L.u.late.B, lane);
    pdy_codes(L.len8, 286u, L.u.late.tab, L.u.late.B, lane);
    pdy_codes(L.len8 + PDY_LL, 30u, L.u.late.tab + PDY_LL, L.u.late.B, lane);
    pdy_codes(L.len8 + PDY_LL + PDY_D, 19u, L.u.late.tab + PDY_LL + PDY_D, L.u.late.B, lane);
    if (lane == 0u) {
        uint32_t hclen = 19u;
        while (hclen > 4u && !L.len8[PDY_LL + PDY_D + pdy_cl_order(hclen - 1u)]) hclen--;
        L.misc[2] = hclen;
    }
    __syncthreads();
    const uint32_t hlit = L.misc[0], hdist = L.misc[1], hclen = L.misc[2], nh = L.misc[3] < PDY_HDR ? L.misc[3] : PDY_HDR;
    // ---- CHOICE ----
    uint32_t fixed_bits = 0u, dyn_bits = 0u;
    for (uint32_t s = lane; s < 286u; s += 64u) {
        fixed_bits += L.cnt[s] * (pdy_fixed_len(s) + pdy_lext(s));
        dyn_bits += L.cnt[s] * (L.len8[s] + pdy_lext(s));
    }
    if (lane < 30u) {
        fixed_bits += L.cnt[PDY_LL + lane] * (5u + pdy_dext(lane));
        dyn_bits += L.cnt[PDY_LL + lane] * (L.len8[PDY_LL + lane] + pdy_dext(lane));
    }
    if (lane < 19u) dyn_bits += L.cnt[PDY_LL + PDY_D + lane] * (L.len8[PDY_LL + PDY_D + lane] + pdy_cext(lane));
    fixed_bits = 3u + pdy_sum(fixed_bits);
    dyn_bits = 17u + 3u * hclen + pdy_sum(dyn_bits);
    const uint32_t tail_bits = t.last ? 0u : 3u, tail_bytes = t.last ? 0u : 4u;
    const uint32_t stored = 5u + len + (t.last ? 0u : 5u);
    const uint32_t fixed_bytes = ((fixed_bits + tail_bits + 7u) >> 3) + tail_bytes, dyn_bytes = ((dyn_bits + tail_bits + 7u) >> 3) + tail_bytes;
    const bool no_stored = (t.flags & DEBIG_PNG_ENCODE_NO_STORED) != 0u;
    bool dyn;
    if (t.flags & DEBIG_PNG_ENCODE_ONLY_DYNAMIC) dyn = (((uint64_t)dyn_bytes + 3u) & ~(uint64_t)3u) <= t.slot_cap;
    else dyn = dyn_bits < fixed_bits && (dyn_bytes < stored || no_stored);
    if (!dyn && fixed_bytes >= stored && !no_stored) return ped_stored(stream + c0, slot, len, t.last, lane);
    // ---- EMIT ----
    uint32_t obits = 0u, carry = 0u, nb = 0u;
    uint64_t bits = 0u;
    if (!dyn) {
        if (lane == 0u) {
            bits = t.last | 2u; /* BFINAL, BTYPE 01 */
            nb = 3u;
        }
        pdy_put(L.u.late.out, ow, obits, carry, bits, nb, lane);
    } else {
        if (lane == 0u) {
            bits = t.last | 4u | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | ((hclen - 4u) << 13); /* BFINAL, BTYPE 10, HLIT, HDIST, HCLEN */
            nb = 17u;
        } else if (lane <= hclen) {
            bits = L.len8[PDY_LL + PDY_D + pdy_cl_order(lane - 1u)] & 7u;
            nb = 3u;
        }
        pdy_put(L.u.late.out, ow, obits, carry, bits, nb, lane);
        for (uint32_t base = 0u; base < nh; base += 64u) {
            nb = 0u;
            bits = 0u;
            if (base + lane < nh) {
                const uint32_t h = L.u.late.hdr[base + lane], sym = h & 31u;
                const uint32_t e = L.u.late.tab[PDY_LL + PDY_D + sym]; /* sym < PDY_CL */
                nb = (e >> 16) + pdy_cext(sym);
                bits = (e & 0xffffu) | ((uint64_t)((h >> 8) & 127u) << (e >> 16));
            }
            pdy_put(L.u.late.out, ow, obits, carry, bits, nb, lane);
        }
    }
    for (uint32_t base = 0u; base <= ntok; base += 64u) {
        nb = 0u;
        bits = 0u;
        const uint32_t i = base + lane;
        if (i <= ntok) bits = pdy_token(L, i < ntok ? row[i] & ~PDY_EOB : PDY_EOB, dyn, nb);
        pdy_put(L.u.late.out, ow, obits, carry, bits, nb, lane);
    }
    return ped_trailer(L.u.late.out, ow, obits, carry, 0u, t.last, lane);
}

__global__ void __launch_bounds__(PED_THREADS)
debig_png_encode_dynamic_kernel(const uint8_t *__restrict__ streams, uint8_t *__restrict__ slots, uint8_t *tokens,
                                const debig_png_encode_dynamic_task *__restrict__ tasks, uint32_t *__restrict__ counts, uint32_t n_tasks)
{
    __shared__ PdyLds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_encode_dynamic_task t = tasks[ti];
        // (uniform over the wavefront: every lane skips, or none)
        if (!pdy_task_ok(t, streams, slots, tokens, counts)) continue;
        uint32_t *row = reinterpret_cast<uint32_t *>(tokens + t.token_off);
        const uint32_t ntok = pdy_match(L, streams + t.stream_off, row, t, lane);
        const uint32_t bytes = pdy_finish(L, streams + t.stream_off, slots + t.slot_off, row, t, ntok, lane);
        if (lane == 0u) counts[t.count_idx] = bytes;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PED_THREADS)
debig_png_encode_codes_kernel(const uint8_t *__restrict__ counts, uint8_t *__restrict__ lens, const debig_png_encode_codes_task *__restrict__ tasks,
                              uint32_t n_tasks)
{
    __shared__ PdyCodesLds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_encode_codes_task t = tasks[ti];
        // (uniform over the wavefront: every lane skips, or none)
        if (t.n == 0u || t.n > 286u || t.limit == 0u || t.limit > 15u || (1u << t.limit) < t.n) continue;
        if (!stage_addr_ok(counts, t.counts_off, 3u) || lens == nullptr) continue;
        const uint32_t *c = reinterpret_cast<const uint32_t *>(counts + t.counts_off);
        bool big = false;
        for (uint32_t s = lane; s < t.n; s += 64u) {
            const uint32_t v = c[s];
            L.cnt[s] = v;
            big |= v > DEBIG_PNG_ENCODE_CODES_MAX_COUNT;
        }
        __syncthreads();
        if (__any(big)) continue;
        pdy_lengths(L.cnt, t.n, t.limit, L.len8, L.B, lane);
        for (uint32_t s = lane; s < t.n; s += 64u) lens[t.lens_off + s] = L.len8[s];
        __syncthreads();
    }
}
