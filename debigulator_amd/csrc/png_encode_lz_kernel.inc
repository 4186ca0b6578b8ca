// png_encode_lz_kernel.inc -- level 3 of the PNG encode (include/decode_png.h: debig_png_encode_batch_lz; include/debig_hip.h has the
// rule word for word: debig_hip_png_encode_lz_batch and its task).
//
// LZ       one wavefront per chunk task.  MATCH is this file's; BUILD, CHOICE and EMIT are level 2's pdy_finish
//          (png_encode_dynamic_kernel.inc), the table and the window level 1's ped_hash / ped_window (png_encode_kernel.inc).
//   MATCH  64 positions per step, one lane each.
//            - The fixed distances 1, bpp, S, S - bpp, S + bpp (S: the task's row_stride) need no table.  For each of them the
//              wavefront keeps an equality bitmap of six 64-bit words, bit x of word j: s[gp] == s[gp - d] at position 64 j + x of
//              the step (0 where gp < d or the position is behind the chunk's end).  The words are wave-uniform values from
//              __ballot; a step shifts them by one word and fills the sixth with ONE coalesced byte compare per distance, 320
//              positions ahead.  A lane's length is the run of ones from its bit: a count of trailing zeros of the first word's
//              complement, plus -- where that word is all ones from the lane on -- the run that starts the second word, which is
//              the same for every lane.  6 x 64 - 63 = 321 >= 258 bits lie in front of the last lane.
//            - Only the table's candidate is extended per lane, and only where the byte that would make it longer than the best
//              fixed distance agrees; four bytes per compare while four are left in front of the chunk's end.
//            - The walk is level 1's with the rule's deferral: a match of 3 .. 15 bytes whose right neighbour in the step has a
//              longer one becomes a literal.
//          A lane whose position starts a token stores it in level 2's format (pdy_step_tokens).
// Every position read from the table is checked before it is an address; a match never reads at or behind the chunk's end or in
// front of the stream's first byte.  No loop waits for another wavefront.  No scratch, no inline assembly.  A task that breaks a
// bound is skipped.
// Included behind png_encode_dynamic_kernel.inc by debig_hip.hip (hipcc) and by the CPU emulator build (tests).

#define PLZ_MAX_LAZY 16u
#define PLZ_DISTS 5u
#define PLZ_WORDS 6u

DEV_INLINE bool plz_task_ok(const debig_png_encode_lz_task &t, const void *streams, const void *slots, const void *tokens, const void *counts)
{
    if (t.level != 3u || t.last > 1u || t.bpp == 0u || t.bpp > 8u) return false;
    if (t.row_stride != 0u && (t.row_stride <= t.bpp || t.row_stride > PED_WINDOW - t.bpp)) return false;
    if (t.chunk_len == 0u || t.chunk_len > DEBIG_PNG_ENCODE_CHUNK) return false;
    if (t.stream_len >= 0xffffffffull || t.chunk_off >= t.stream_len || t.chunk_len > t.stream_len - t.chunk_off) return false;
    if ((uint64_t)t.slot_cap < DEBIG_PNG_ENCODE_SLOT(t.chunk_len) || t.token_cap / 4u < t.chunk_len) return false;
    return stage_addr_ok(slots, t.slot_off, 3u) && stage_addr_ok(tokens, t.token_off, 3u) && stage_addr_ok(counts, 0u, 3u) && streams != nullptr;
}

// the equality bits of the 64 chunk positions from x0 at distance d (0: none); cur: this lane's byte, in: its position is in the chunk
DEV_INLINE unsigned long long plz_word(const uint8_t *__restrict__ stream, uint32_t c0, uint32_t d, uint32_t x0, uint32_t cur, bool in, uint32_t lane)
{
    bool e = false;
    if (in && d != 0u && c0 + x0 + lane >= d) e = stream[c0 + x0 + lane - d] == cur;
    return __ballot(e);
}

// how many bytes at a and at b agree, at most maxl; four at a time
DEV_INLINE uint32_t plz_match_len(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t maxl)
{
    uint32_t l = 0u;
    while (l + 4u <= maxl) {
        uint32_t x, y;
        __builtin_memcpy(&x, a + l, 4);
        __builtin_memcpy(&y, b + l, 4);
        if (x != y) return l + ((uint32_t)__builtin_ctz(x ^ y) >> 3);
        l += 4u;
    }
    while (l < maxl && a[l] == b[l]) l++;
    return l;
}

// MATCH of level 3 -> the tokens in the row
DEV_INLINE uint32_t plz_match(PdyLds &L, const uint8_t *__restrict__ stream, uint32_t *row, const debig_png_encode_lz_task &t, uint32_t lane)
{
    const uint32_t len = t.chunk_len, c0 = (uint32_t)t.chunk_off, bpp = t.bpp, S = t.row_stride;
    for (uint32_t k = lane; k < PDY_SYMS; k += 64u) L.cnt[k] = 0u;
    ped_window(L.u.hash, stream, c0, t.stream_len, lane);
    // the fixed distances in the rule's order; 0: none, or equal to an earlier one
    uint32_t fd[PLZ_DISTS];
    fd[0] = 1u;
    fd[1] = bpp > 1u ? bpp : 0u;
    fd[2] = S;
    fd[3] = (S != 0u && S - bpp != 1u && S - bpp != bpp) ? S - bpp : 0u;
    fd[4] = S != 0u ? S + bpp : 0u;
    unsigned long long w[PLZ_DISTS][PLZ_WORDS];
DEV_UNROLL
    for (uint32_t j = 0u; j + 1u < PLZ_WORDS; j++) {
        const uint32_t x = 64u * j + lane;
        const bool in = x < len;
        const uint32_t cur = in ? stream[c0 + x] : 0u;
DEV_UNROLL
        for (uint32_t k = 0u; k < PLZ_DISTS; k++) w[k][j + 1u] = plz_word(stream, c0, fd[k], 64u * j, cur, in, lane);
    }
    uint32_t covered = 0u, ntok = 0u;
    for (uint32_t base = 0u; base < len; base += 64u) {
        const uint32_t p = base + lane, gp = c0 + p;
        const uint32_t maxl = p < len ? (len - p < PED_MAX_MATCH ? len - p : PED_MAX_MATCH) : 0u;
        {
            const uint32_t x0 = base + 64u * (PLZ_WORDS - 1u);
            const bool in = x0 + lane < len;
            const uint32_t cur = in ? stream[c0 + x0 + lane] : 0u;
DEV_UNROLL
            for (uint32_t k = 0u; k < PLZ_DISTS; k++) {
DEV_UNROLL
                for (uint32_t j = 0u; j + 1u < PLZ_WORDS; j++) w[k][j] = w[k][j + 1u];
                w[k][PLZ_WORDS - 1u] = plz_word(stream, c0, fd[k], x0, cur, in, lane);
            }
        }
        uint32_t h = 0u, cand = 0u;
        if (maxl >= 3u) {
            h = ped_hash(stream + gp);
            cand = L.u.hash[h];
        }
        __syncthreads(); /* every lane has read before any inserts */
        if (maxl >= 3u) atomicMax(&L.u.hash[h], gp + 1u);
        uint32_t best = 0u, dist = 0u;
        const bool open = maxl >= 3u && p >= covered;
DEV_UNROLL
        for (uint32_t k = 0u; k < PLZ_DISTS; k++) {
            if (fd[k] == 0u) continue; /* (uniform) */
            // the run of ones that starts the second word: the same for every lane
            uint32_t tail = 0u;
            bool on = true;
DEV_UNROLL
            for (uint32_t j = 1u; j < PLZ_WORDS; j++) {
                const unsigned long long z = ~w[k][j];
                if (on) tail += z ? (uint32_t)__builtin_ctzll(z) : 64u;
                on = on && z == 0ull;
            }
            const unsigned long long z0 = ~w[k][0] >> lane;
            uint32_t l = z0 ? (uint32_t)__builtin_ctzll(z0) : 64u - lane + tail;
            if (l > maxl) l = maxl;
            if (open && l > best) {
                best = l;
                dist = fd[k];
            }
        }
        if (open) {
            // the table's candidate: a position in front of this one, inside the stream and inside the window; it can only win
            // where it agrees in the byte behind the best so far
            if (cand != 0u && cand - 1u < gp && gp - (cand - 1u) <= PED_WINDOW && best < maxl) {
                const uint32_t d = gp - (cand - 1u);
                if (stream[gp - d + best] == stream[gp + best]) {
                    const uint32_t l = plz_match_len(stream + gp - d, stream + gp, maxl);
                    if (l > best) {
                        best = l;
                        dist = d;
                    }
                }
            }
            if (best < 3u || (best == 3u && dist > PED_TOO_FAR)) best = 0u;
        }
        L.lens[lane] = best;
        __syncthreads();
        // the walk, the same in every lane: greedy, and a short match gives way to a longer one at its right neighbour
        uint32_t q = covered - base; /* covered >= base: a step covers at least its own 64 positions */
        unsigned long long starts = 0ull, literal = 0ull;
        while (q < 64u && base + q < len) {
            starts |= 1ull << q;
            uint32_t l = L.lens[q];
            if (l >= 3u && l < PLZ_MAX_LAZY && q != 63u && base + q + 1u < len && L.lens[q + 1u] > l) {
                literal |= 1ull << q;
                l = 0u;
            }
            q += l ? l : 1u;
        }
        covered = base + q;
        if ((literal >> lane) & 1ull) best = 0u;
        pdy_step_tokens(L, row, t.token_cap, starts, ntok, best, dist, stream + gp, lane);
    }
    return ntok;
}

__global__ void __launch_bounds__(PED_THREADS)
debig_png_encode_lz_kernel(const uint8_t *__restrict__ streams, uint8_t *__restrict__ slots, uint8_t *tokens,
                           const debig_png_encode_lz_task *__restrict__ tasks, uint32_t *__restrict__ counts, uint32_t n_tasks)
{
    __shared__ PdyLds L;
    const uint32_t lane = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_encode_lz_task t = tasks[ti];
        // (uniform over the wavefront: every lane skips, or none)
        if (!plz_task_ok(t, streams, slots, tokens, counts)) continue;
        uint32_t *row = reinterpret_cast<uint32_t *>(tokens + t.token_off);
        const uint32_t ntok = plz_match(L, streams + t.stream_off, row, t, lane);
        const uint32_t bytes = pdy_finish(L, streams + t.stream_off, slots + t.slot_off, row, t, ntok, lane);
        if (lane == 0u) counts[t.count_idx] = bytes;
        __syncthreads();
    }
}
