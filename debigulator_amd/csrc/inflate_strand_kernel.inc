// inflate_strand_kernel.inc -- the throughput path, second generation: LONG per-lane segments.
//
// The scan of inflate_split_kernel.inc cuts a 4.4 KB staged window into 64 segments of 68 bytes and
// every lane guesses where its segment's first symbol starts.  Measured on 64 KiB fixed-Huffman
// streams (profiles/r03_pmc_split_fixed.txt, r03_phases_split_fixed.txt): 9 windows x 63 guesses per
// stream, every symbol decoded 2.36 times (a positions-only round that starts 272 bits early, a full
// round, and redo rounds that cost a whole segment whatever the number of lanes in them), 42.7 of 64
// lanes active (a round lasts as long as its densest segment), 137 k wave-instructions per stream.
// What bounded it was the SHAPE: segment length tied to an LDS window, one guess per 544 bits.
//
// Here a lane owns a STRAND: a contiguous piece of the block as long as the block allows (a 64 KiB
// fixed-Huffman stream is ONE window of 64 strands of ~580 bytes; a dynamic block is sized from the
// block before it).  Nothing is staged for the whole wavefront: every lane keeps a 64-byte RING of
// its own input in LDS (19 dwords per lane: 16 + the first three again, so the 64-bit window read
// never wraps) and refills the 16-byte quads it has consumed from global memory between phases.
//
//   lead      lanes 1..63 start ST_LEAD_BITS before their strand and chase positions only (lenient:
//             nothing stops a lane that decodes garbage) until they are inside it;
//   main      ONE pass: every lane decodes its strand in PHASES of 15 symbol slots, all lanes in lock
//             step (a lane that cannot go on -- ring limit, end of strand -- emits no-ops), keeping
//             what it decodes: a phase leaves one UNIT of 16 words per lane {header, 15 tokens} and the
//             64 lanes store one coalesced 4 KB unit row.  The scan is lenient; the first terminal
//             event (end of block, errors, the tail gate Q2) is frozen beside it, as in the 68-byte scan;
//   chain     lane L is right when it started where lane L - 1 ended.  A lane that was not (about one
//             in eight after a 272-bit lead) is decoded again from its true start, but only until
//             it reaches the position where its first decode began unit ST_SYNC_UNIT: from there on
//             the two decodes are the same symbols.  The re-decoded tokens go to PATCH units; the
//             segment's token sequence is patch units ++ first-decode units from ST_SYNC_UNIT on.
//             (A lane that has not fallen into step by then is decoded to its end: 1e-4 of lanes.)
//
// The LZ77 half (lz_body of inflate_split_kernel.inc) replays a window unit by unit: a unit carries
// its own output offset, so 64 lanes place 64 consecutive units of the stream into the tile with
// straight-line code (15 tokens from registers), then the far / near match machinery runs unchanged.
//
// What it replaces in the reference: src/inflate.c:786-1965, same observable behaviour as
// debig_inflate_kernel; streams that do not fit their workspace share go to debig_inflate_kernel
// (DEBIG_CLASS_RETRY) as in the 68-byte path.

#ifndef ST_LEAD_BITS
#define ST_LEAD_BITS 272u /* strands shorter than ST_REBALANCE_MIN_BITS */
#endif
#ifndef ST_LEAD_BITS_LONG
#define ST_LEAD_BITS_LONG 544u /* longer strands: fewer lanes arrive out of step (one in twelve), and twice the sample for the
                                  density estimate (64 KiB text streams: 26 -> 23 main phases; 20 would be even) */
#endif
#ifndef ST_SYNC_UNIT
#define ST_SYNC_UNIT 4u /* a re-decoded lane joins its first decode at the start of this unit */
#endif
#define ST_UNIT_TOK 15u  /* tokens per unit (+ the header word = 64 bytes) */
#define ST_UNIT_ROWS 16u /* 256-byte workspace rows per unit row (64 lanes x 64 bytes) */
#define ST_INFO_ROWS 4u  /* per window: nbytes | units | patch adjustment | (spare) */
#define ST_RING_DW 16u
#define ST_SLOT_DW 19u /* ring + 3 mirror dwords; odd: lanes spread over the LDS banks */
#ifndef ST_SEG_MIN
#define ST_SEG_MIN 64u /* bytes; >= (ST_LEAD_BITS + 127) / 8 rounded to 16 */
#endif
#ifndef ST_SEG_MAX
#define ST_SEG_MAX 768u /* bytes: a strand's output offset must fit 20 bits (8 * 768 / 2 * 258 < 2^20) */
#endif
#ifndef ST_REBALANCE
#define ST_REBALANCE 1 /* strands cut again by the symbol densities the lead measured */
#endif
#define ST_REBALANCE_MIN_BITS 2048u /* ... in windows whose strands are at least this long */
#define ST_STRAND_MAX 896u /* bytes: the longest strand after that (8 * 896 / 2 * 258 < 2^20: the unit header's offset field) */
#ifndef ST_DYN_FIRST_GUESS
#define ST_DYN_FIRST_GUESS 16384u /* compressed bytes assumed for the first dynamic block of a stream */
#endif
#ifndef ST_PROBE_UNITS
#define ST_PROBE_UNITS 3u /* short blocks: lane 0 alone looks this far for the end of the block */
#endif
#define TOK_NOP 0x40000000u /* nothing (a lane that could not go on, the slot of a terminal event) */
/* REC_WIN2 (declared in inflate_split_kernel.inc), a strand window: row = info rows, a = lanes used | flag << 8,
 * b = status of FL_ERR, c = output bytes, d = main unit rows | patch unit rows << 20 | workspace rows per unit row << 40 */

struct __attribute__((aligned(16))) StrandLds {
    static constexpr int NW = 1;
    static constexpr uint32_t WIN_B = 464; /* block headers go through the shared helpers: 512 staged bytes */
    typedef Fmt16 Fmt;
    CodeTabsT<TabCfg<1>::PBL, uint16_t, 256u> t;
    union {
        uint32_t ring[64u * ST_SLOT_DW]; /* symbol windows: 76 bytes per lane */
        struct {                         /* block headers (the rings are idle then) */
            uint32_t inwin[(464 + 48) / 4];
            uint8_t lens[320 + 144];
            uint16_t cl_tab[1 << 7];
            uint32_t cl_len[19];
            uint32_t cl_code[19];
            uint32_t cl_used[19];
        };
    };
};

#ifdef DEBIG_EMU
DEV_INLINE void st_store_unit16(uint32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
DEV_INLINE void st_load_unit16(const uint32_t *p, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) { a = p[0]; b = p[1]; c = p[2]; d = p[3]; }
#else
typedef uint32_t st_u32x4 __attribute__((ext_vector_type(4)));
DEV_INLINE void st_store_unit16(uint32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    st_u32x4 v = {a, b, c, d};
#if defined(ST_UNIT_STORE_NT) && ST_UNIT_STORE_NT
    __builtin_nontemporal_store(v, reinterpret_cast<st_u32x4 *>(p));
#else
    *reinterpret_cast<st_u32x4 *>(p) = v; /* 16 bytes of a 64-byte unit at a time: L2 has to merge them (streamed, every piece was a partial write to memory) */
#endif
}
DEV_INLINE void st_load_unit16(const uint32_t *p, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d)
{
    const st_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const st_u32x4 *>(p));
    a = v[0]; b = v[1]; c = v[2]; d = v[3];
}
#endif

// 16 input bytes at stream-relative byte idx (idx + in is 16-byte aligned); bytes outside [0, in_len)
// read as zero (the reference reads whatever follows its input: only corrupt streams can tell)
DEV_NOINLINE uint4 st_load16_edge(const uint8_t *in, uint64_t in_len, int64_t idx)
{
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; k++) {
        const int64_t i = idx + k;
        if (i >= 0 && (uint64_t)i < in_len) w[k >> 2] |= (uint32_t)in[i] << (8 * (k & 3));
    }
    uint4 v;
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}
DEV_INLINE uint4 st_load16(const uint8_t *in, uint64_t in_len, int64_t idx)
{
    if (idx >= 0 && (uint64_t)idx + 16u <= in_len) return ld_global_u4(in + idx);
    return st_load16_edge(in, in_len, idx); /* the first / last bytes of a stream: out of line */
}

// per-lane decode state.  Bit positions are relative to the lane's ORIGIN, a 16-byte aligned address
// at or below the byte it started from (`org`: its stream-relative byte index).
struct StLane {
    uint32_t lp;     /* next symbol */
    uint32_t bound;  /* a symbol may start at positions < bound (strand end, tail gate, ring) */
    uint32_t nbytes; /* output bytes of the tokens so far (lenient: counts on behind a terminal event) */
    uint32_t w0;     /* the ring holds dwords [w0, wv) of the lane's input (both multiples of 4, wv <= w0 + 16) */
    uint32_t wv;
    uint32_t np;     /* quads on their way from memory: dwords [wv, wv + 4 np), written to the ring by the next refill */
    int64_t org;
    uint4 pq[3];
};
struct StTerm { /* the first terminal event since the record was armed */
    uint32_t ts;   /* FL_* | status << 8; 0 = none */
    uint32_t tend; /* where strict decoding stopped (lane relative) */
    uint32_t fznb; /* nbytes then */
    uint32_t at;   /* unit | slot << 16 */
};
DEV_INLINE void st_term_clear(StTerm &t) { t.ts = 0; t.tend = 0; t.fznb = 0; t.at = 0; }

DEV_INLINE void st_ring_init(uint32_t *rg, const uint8_t *in, uint64_t in_len, int64_t sbit, StLane &a, int active)
{
    const int64_t sb = sbit >> 3;
    const uintptr_t ga = (uintptr_t)(in + sb);
    a.org = sb - (int64_t)(ga & 15u);
    a.lp = (uint32_t)(sbit - 8 * a.org);
    a.w0 = 0;
    a.wv = 16;
    a.np = 0;
    if (active) {
DEV_UNROLL
        for (uint32_t q = 0; q < 4; q++) {
            const uint4 v = st_load16(in, in_len, a.org + 16 * (int64_t)q);
            rg[4 * q] = v.x; rg[4 * q + 1] = v.y; rg[4 * q + 2] = v.z; rg[4 * q + 3] = v.w;
            if (q == 0) { rg[16] = v.x; rg[17] = v.y; rg[18] = v.z; }
        }
    }
}
// A lane's input comes from memory at the latency of a miss (32768 lanes per XCD read 32768 sequential streams: no
// cache holds a line until its lane comes back to it), so the ring is refilled from REGISTERS: at the START of a
// phase the three quads that follow the ring are asked for (st_ring_fetch: they have the whole phase to arrive),
// at its END those whose ring slots the lane has left behind go in (st_ring_commit: at most three: a phase cannot
// pass the ring's limit by more than one symbol); what was fetched and not needed yet is fetched again.  The
// ring is whole at the start of every phase: 11..14 dwords ahead of the lane.  (Only the lane touches its ring:
// no barrier anywhere.)
DEV_INLINE void st_ring_fetch(const uint8_t *in, uint64_t in_len, StLane &a, int active)
{
    if (active) {
DEV_UNROLL
        for (uint32_t i = 0; i < 3; i++) a.pq[i] = st_load16(in, in_len, a.org + 4 * (int64_t)(a.wv + 4u * i));
    }
    a.np = active ? 3u : 0u;
}
DEV_INLINE void st_ring_commit(uint32_t *rg, StLane &a, int active)
{
    const uint32_t w1 = active ? ((a.lp >> 5) & ~3u) : a.w0; /* the quads below the lane's position are free */
    uint32_t k = (w1 - a.w0) >> 2;
    k = k < a.np ? k : a.np;
DEV_UNROLL
    for (uint32_t i = 0; i < 3; i++) {
        if (i < k) {
            const uint32_t p = (a.wv + 4u * i) & 15u;
            rg[p] = a.pq[i].x; rg[p + 1] = a.pq[i].y; rg[p + 2] = a.pq[i].z; rg[p + 3] = a.pq[i].w;
            if (p == 0) { rg[16] = a.pq[i].x; rg[17] = a.pq[i].y; rg[18] = a.pq[i].z; }
        }
    }
    a.w0 += 4u * k;
    a.wv += 4u * k;
    a.np = 0;
}
DEV_INLINE uint32_t st_ring_bound(const StLane &a) { return 32u * (a.wv - 2u); }

DEV_INLINE Win64 st_win64(const uint32_t *rg, uint32_t lp)
{
    const uint32_t w = (lp >> 5) & 15u, sh = lp & 31u;
    const uint32_t d0 = rg[w], d1 = rg[w + 1], d2 = rg[w + 2];
    Win64 r;
    r.lo = funnel32(d1, d0, sh);
    r.hi = funnel32(d2, d1, sh);
    return r;
}

// the lead: positions only, lenient (scan_positions16 of inflate_split_kernel.inc on the ring)
DEV_INLINE void st_step_lead(const StrandLds &S, const uint32_t *rg, StLane &a, const uint32_t lm, const uint32_t dm, uint32_t &nsym)
{
    if (a.lp < a.bound) {
        nsym++;
        const Win64 wb = st_win64(rg, a.lp);
        uint32_t e = S.t.lit_tab[wb.lo & lm];
        const uint32_t l = E16_LEN(e), n1 = l + E16_X(e);
        uint32_t de = S.t.dist_tab[funnel32(wb.hi, wb.lo, n1) & dm];
        const uint32_t m = E16_LENMASK(e);
        const uint32_t y = D16_TOTAL(de) & m;
        if (umin32(l, y | ~m) == 0) {
            if ((e & 0x1fu) == 0x10u) { a.lp += E16_SPECIAL_LEN(e); return; } /* end of block | 286 / 287 */
            if (e == 0u) { a.lp += 1u; return; }
            if (l != 0u && (de == 0u || (de & 0x8ffu) == 0x800u)) { a.lp += n1 + (de == 0u ? 1u : (de >> 12) & 15u); return; }
            // long codes (or what hides behind them)
            if (Fmt16::is_link(e) || Fmt16::is_slow(e)) e = huff_slow(wb.lo, S, CODE_LIT, e);
            if (e == 0) { a.lp += 1u; return; }
            if (E16_LEN(e) == 0) { a.lp += E16_SPECIAL_LEN(e); return; }
            const uint32_t l2 = E16_LEN(e), n2 = l2 + E16_X(e);
            a.lp += n2;
            if (E16_ISLEN(e)) {
                const uint32_t bits2 = funnel32(wb.hi, wb.lo, n2);
                de = S.t.dist_tab[bits2 & dm];
                if (Fmt16::is_link(de) || Fmt16::is_slow(de)) de = huff_slow(bits2, S, CODE_DIST, de);
                if (de == 0) a.lp += 1u;
                else if (D16_BAD(de)) a.lp += (de >> 12) & 15u;
                else a.lp += D16_TOTAL(de);
            }
            return;
        }
        a.lp += n1 + y;
    }
}

// One symbol with every rare case handled (scan_step_general_tok of inflate_split_kernel.inc): codes longer
// than the direct tables, no code at all, end of block, symbols 286 / 287, distance symbols 30 / 31.  OUT OF LINE
// on purpose: a phase is fifteen copies of the symbol step, and with this path inlined in each of them the kernel
// was 300 KB of code (several times the instruction cache).  Pure: what the event means for the lane is the
// caller's business.
#ifdef DEBIG_EMU
#define ST_NOUNROLL
#else
#define ST_NOUNROLL _Pragma("nounroll")
#endif
struct StGen {
    uint32_t lp;     /* behind the symbol (lenient: behind what a guessing lane skips) */
    uint32_t tok;    /* TOK_NOP unless a literal / match came out */
    uint32_t outlen;
    uint32_t ts;     /* terminal event: FL_* | status << 8, 0 = none */
    uint32_t tend;   /* where strict decoding stops then */
};
DEV_NOINLINE StGen st_general_slow(const StrandLds *Sp, const uint32_t lo, const uint32_t hi, const uint32_t lp0)
{
    const StrandLds &S = *Sp;
    StGen r;
    r.lp = lp0; r.tok = TOK_NOP; r.outlen = 0; r.ts = 0; r.tend = 0;
    const uint32_t bits = lo;
    uint32_t e = S.t.lit_tab[bits & S.t.mask[CODE_LIT]];
    if (Fmt16::is_link(e) || Fmt16::is_slow(e)) e = huff_slow(bits, S, CODE_LIT, e);
    if (e == 0) { /* no code */
        r.ts = (uint32_t)FL_ERR | ((uint32_t)DEBIG_E_NO_CODE << 8);
        r.tend = r.lp;
        r.lp += 1u;
    } else if (E16_LEN(e) == 0) { /* end of block | symbols 286 / 287 */
        const uint32_t x = E16_X(e);
        r.lp += E16_SPECIAL_LEN(e);
        r.ts = x == 1u ? (uint32_t)FL_EOB : ((uint32_t)FL_ERR | ((uint32_t)DEBIG_E_LITLEN_286_287 << 8));
        r.tend = r.lp;
    } else {
        const uint32_t l = E16_LEN(e), nx = E16_X(e), is_len = E16_ISLEN(e);
        const uint32_t vv = E16_V(e) + ((bits >> l) & ((1u << nx) - 1u)); /* the byte | length - 3 */
        r.lp += l + nx;
        if (is_len) {
            const uint32_t bits2 = funnel32(hi, lo, l + nx);
            uint32_t de = S.t.dist_tab[bits2 & S.t.mask[CODE_DIST]];
            if (Fmt16::is_link(de) || Fmt16::is_slow(de)) de = huff_slow(bits2, S, CODE_DIST, de);
            if (de == 0 || D16_BAD(de)) { /* no code | distance symbol 30 / 31 */
                r.ts = (uint32_t)FL_ERR | ((de == 0 ? (uint32_t)DEBIG_E_NO_CODE : (uint32_t)DEBIG_E_DIST_SYMBOL) << 8);
                r.tend = r.lp;
                r.lp += de == 0 ? 1u : (de >> 12) & 15u;
            } else {
                const uint32_t dx = D16_EXTRA(de), ld = D16_TOTAL(de) - dx;
                const uint32_t dm1 = (D16_M(de) << dx) + ((bits2 >> ld) & ((1u << dx) - 1u));
                r.lp += ld + dx;
                r.tok = TOK_MATCH | (vv << 16) | dm1;
                r.outlen = vv + 3u;
            }
        } else {
            r.tok = vv;
            r.outlen = 1u;
        }
    }
    return r;
}

// one symbol slot of a phase: the token (TOK_NOP when the lane cannot go on).
// STRICT = false (main pass): a terminal event is recorded in TA / TB if they are armed, the rest of the unit
// is blanked (cut) and the lane goes on leniently; STRICT = true (a lane decoding from its true position): the
// lane stops.
template <bool STRICT>
DEV_INLINE uint32_t st_step(const StrandLds &S, const uint32_t *rg, StLane &a, StTerm &TA, StTerm &TB, const uint32_t at,
                            const uint32_t lm, const uint32_t dm, const uint32_t sync_at, uint32_t &synced, uint32_t &cut,
                            uint32_t &cutnb)
{
    uint32_t tokv = TOK_NOP;
    if (STRICT && a.bound != 0 && a.lp == sync_at) { /* the lane's first decode began a unit exactly here: the same symbols follow
                                                        (bound == 0: the lane has stopped at a terminal event -- where the lenient first
                                                        decode went on from is no place to join it) */
        synced = 1u;
        a.bound = 0;
    }
    // (Measured and not kept, profiles/r04_strand_notes.txt: the plain symbol decoded by every lane in straight-line code and
    // taken by selects, no exec-mask bookkeeping in the hot path: 0.909 ms against 0.890 -- the lanes that cannot go on then
    // load the LDS pipe for nothing.)
    if (a.lp < a.bound) {
        const Win64 wb = st_win64(rg, a.lp);
        const uint32_t e = S.t.lit_tab[wb.lo & lm];
        const uint32_t l = E16_LEN(e), nx = E16_X(e);
        const uint32_t n1 = l + nx;
        const uint32_t bits2 = funnel32(wb.hi, wb.lo, n1);
        const uint32_t de = S.t.dist_tab[bits2 & dm];
        const uint32_t m = E16_LENMASK(e);
        const uint32_t dtot = D16_TOTAL(de), y = dtot & m;
        if (umin32(l, y | ~m) == 0) {
            // Codes longer than the direct tables are what real encoders' tables are made of (about 1 % of the
            // symbols of a photo PNG: with 64 lanes in step most slots have a lane on one): one more look-up for the
            // literal / length code and one for the distance code, right here.  What is left after that -- end of
            // block, no code, symbols 286 / 287, distance symbols 30 / 31, tables too large for second levels --
            // goes out of line.
            uint32_t e2 = e;
            if (Fmt16::is_link(e2))
                e2 = S.t.sub_tab[Fmt16::link_base(e2) + ((wb.lo >> TabCfg<1>::PBL) & ((1u << Fmt16::link_k(e2)) - 1u))];
            const uint32_t l2 = E16_LEN(e2), nx2 = E16_X(e2), n12 = l2 + nx2;
            const uint32_t bits22 = funnel32(wb.hi, wb.lo, n12);
            uint32_t de2 = S.t.dist_tab[bits22 & dm];
            if (Fmt16::is_link(de2))
                de2 = S.t.sub_tab[Fmt16::link_base(de2) + ((bits22 >> PB_DIST) & ((1u << Fmt16::link_k(de2)) - 1u))];
            const uint32_t m2 = E16_LENMASK(e2);
            const uint32_t dtot2 = D16_TOTAL(de2), y2 = dtot2 & m2;
            if (umin32(l2, y2 | ~m2) != 0) {
                const uint32_t vv = E16_V(e2) + ((wb.lo >> l2) & ((1u << nx2) - 1u));
                const uint32_t dx = D16_EXTRA(de2);
                const uint32_t dm1 = (D16_M(de2) << dx) + ((bits22 >> (dtot2 - dx)) & ((1u << dx) - 1u));
                a.lp += n12 + y2;
                tokv = (vv & ~m2) | ((TOK_MATCH | (vv << 16) | dm1) & m2);
                a.nbytes += 1u + ((vv + 2u) & m2);
            } else {
                const StGen r = st_general_slow(&S, wb.lo, wb.hi, a.lp);
                a.lp = r.lp;
                tokv = r.tok;
                if (r.ts) {
                    int fired = 0;
                    if (TA.ts == 0) { TA.ts = r.ts; TA.tend = r.tend; TA.fznb = a.nbytes; TA.at = at; fired = 1; }
                    if (!STRICT && TB.ts == 0) { TB.ts = r.ts; TB.tend = r.tend; TB.fznb = a.nbytes; TB.at = at; fired = 1; }
                    if (STRICT) { a.lp = r.tend; a.bound = 0; }
                    else if (fired && !cut) { cut = 1u; cutnb = a.nbytes; }
                }
                a.nbytes += r.outlen;
            }
        } else {
            const uint32_t vv = E16_V(e) + ((wb.lo >> l) & ((1u << nx) - 1u));
            const uint32_t dx = D16_EXTRA(de);
            const uint32_t dm1 = (D16_M(de) << dx) + ((bits2 >> (dtot - dx)) & ((1u << dx) - 1u));
            a.lp += n1 + y;
            tokv = (vv & ~m) | ((TOK_MATCH | (vv << 16) | dm1) & m);
            a.nbytes += 1u + ((vv + 2u) & m);
        }
        if (!STRICT) tokv = cut ? TOK_NOP : tokv; /* behind a terminal event recorded in this unit */
    }
    return tokv;
}

// One phase: 15 symbol slots and the header {output offset of the unit inside the lane's decode (20 bits) |
// output bytes of its valid tokens << 20} = one unit of 16 words, tokens first, kept in registers and handed back
// (t[15] = header): the caller stores the 64 bytes in one go -- pieces stored as they were ready were partial
// writes spread over a phase, and every wait for the ring's loads then also waited for a store just issued.
// Main pass (STRICT = false): tokens behind a terminal event recorded in this unit are blanked (what follows such
// an event only counts when the event was a guessing lane's, and then the unit is replaced by a patch unit anyway).
template <bool STRICT>
DEV_INLINE void st_phase(const StrandLds &S, const uint32_t *rg, StLane &a, StTerm &TA, StTerm &TB, const uint32_t u,
                         const uint32_t sync_at, uint32_t &synced, uint32_t t[16])
{
    const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
    const uint32_t nb0 = a.nbytes;
    uint32_t cut = 0, cutnb = 0;
DEV_UNROLL
    for (uint32_t k = 0; k < ST_UNIT_TOK; k++)
        t[k] = st_step<STRICT>(S, rg, a, TA, TB, u | ((k + 1u) << 16), lm, dm, sync_at, synced, cut, cutnb);
    t[15] = (nb0 & 0xfffffu) | (((cut ? cutnb : a.nbytes) - nb0) << 20);
}
DEV_INLINE void st_store_unit(uint32_t *p, const uint32_t t[16])
{
    st_store_unit16(p, t[0], t[1], t[2], t[3]);
    st_store_unit16(p + 4, t[4], t[5], t[6], t[7]);
    st_store_unit16(p + 8, t[8], t[9], t[10], t[11]);
    st_store_unit16(p + 12, t[12], t[13], t[14], t[15]);
}

// lane-relative limits of a lane whose origin is a.org: strand end hi_w (window relative; worg = the
// window origin's stream-relative byte), tail gate (src/inflate.c:1702: symbols may start at
// positions <= 8 (in_len - 1) only)
DEV_INLINE uint32_t st_rel(int64_t pos_w, int64_t worg, int64_t org)
{
    const int64_t v = pos_w - 8 * (org - worg);
    return v < 0 ? 0u : (v > 0x7ffffff0 ? 0x7ffffff0u : (uint32_t)v);
}
DEV_INLINE uint32_t st_gate(uint64_t in_len, int64_t org)
{
    const int64_t tl = 8 * ((int64_t)in_len - 1) - 8 * org; /* last position a symbol may start at */
    return tl < 0 ? 0u : (tl > 0x7ffffff0 ? 0x7ffffff0u : (uint32_t)tl + 1u);
}

// The scan of one stream: block headers and tables as scan_body, symbol windows as described above.
DEV_INLINE void strand_scan_body(StrandLds &S, const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                                 const debig_stream &st, const uint32_t sid, const uint32_t *__restrict__ fixed_tabs,
                                 debig_ws_slot *__restrict__ slots, debig_ws_rec *__restrict__ recs,
                                 uint32_t *__restrict__ rows, debig_result *results, uint32_t *state_out,
                                 volatile uint32_t *publish = nullptr /* debig_strand_pipe_kernel: records complete so far */)
{
    *state_out = DEBIG_E_RETRY;
    PROF_DECL
    const uint32_t lane = lane_id();
    const debig_ws_slot slot = slots[sid];
    const uint8_t *in = in_arena + st.in_off;
    const uint64_t in_len = st.in_len;
    uint8_t *out = out_arena + st.out_off;
    debig_ws_rec *myrec = recs + slot.rec0;
    uint32_t *myrows = rows + slot.row0 * 64u;
    uint32_t *rg = S.ring + lane * ST_SLOT_DW;

    uint32_t status = DEBIG_OK, final_set = 0;
    uint32_t n_blocks = 0, n_windows = 0, n_rounds = 0;
    int64_t end_bits = 0;
    int tables = 0;
    int64_t staged_base = 0;
    int staged_valid = 0;
    int short_mode = 0;
    uint64_t outpos = 0;
    uint32_t row_cur = 0, rec_cur = 0;
    const uint32_t rec_lim = slot.recs ? slot.recs - 1u : 0u;
    uint32_t blk_guess = 0; /* compressed bytes the next Huffman block probably has (0: no block seen yet) */

#define ST_EMIT(KIND, ROW, A, B, C, D)                                                           \
    do {                                                                                         \
        if (rec_cur >= rec_lim) { status = DEBIG_E_RETRY; }                                      \
        else {                                                                                   \
            if (lane == 0) {                                                                     \
                debig_ws_rec rr;                                                                 \
                rr.kind = (KIND); rr.row = (ROW); rr.a = (A); rr.b = (B); rr.c = (C); rr.d = (D); \
                myrec[rec_cur] = rr;                                                             \
            }                                                                                    \
            rec_cur++;                                                                           \
            if (publish) { /* the record, its units and info rows: in L2 before the other wavefront hears of it */ \
                wave_mem_fence();                                                                \
                wave_local_sync();                                                               \
                if (lane == 0) *publish = rec_cur;                                               \
            }                                                                                    \
        }                                                                                        \
    } while (0)

    if (slot.recs == 0) return;
    if (!(st.flags & DEBIG_STREAM_NO_REF_GATES)) {
        if (st.out_cap < in_len) status = DEBIG_E_GATE_RECIPIENT_SMALL;
        else if (in_len < 5) status = DEBIG_E_GATE_INPUT_SHORT;
    }
    if (status == DEBIG_OK) {
        final_set = 1;
        int64_t bitpos = 0;
        int more = 1;
        while (more && status == DEBIG_OK) {
            // ---- block header (as scan_body / debig_inflate_kernel)
            PROF_BEGIN();
            int64_t wbase = stage_window_cached(S, in, in_len, bitpos >> 3, DEBIG_HEADER_NEED, 0, staged_base, staged_valid);
            int64_t org = 8 * wbase;
            BitRd hb;
            br_init(hb, S, bitpos, org);
            br_ensure(hb, S);
            uint32_t bfinal = br_take(hb, 1);
            uint32_t btype = br_take(hb, 2);
            if (bfinal) more = 0;
            n_blocks++;
            if (btype == 3) { bitpos = hb.pos; continue; } /* Q5 */
            if (btype == 0) {
                int64_t p = (hb.pos + 7) & ~(int64_t)7;
                br_init(hb, S, p, org);
                br_ensure(hb, S);
                uint32_t len = br_take(hb, 16);
                br_ensure(hb, S);
                uint32_t nlen = br_take(hb, 16);
                if ((len ^ nlen) != 0xffffu) { status = DEBIG_E_STORED_NLEN; break; }
                if (outpos + len > st.out_cap) { status = DEBIG_E_OUTPUT_FULL; break; }
                ST_EMIT(REC_STORED, 0u, 0u, 0u, (uint64_t)len, (uint64_t)(hb.pos >> 3));
                if (status != DEBIG_OK) break;
                stored_copy<1>(in, in_len, hb.pos >> 3, out + outpos, len);
                outpos += len;
                bitpos = hb.pos + 8 * (int64_t)len;
                continue;
            }
            const int fixed = (btype == 1);
            const int need_p2 = st.p2_on && ((int64_t)outpos > st.p2_s0);
            if (fixed) {
                if (tables != 1) {
                    wave_local_sync();
                    uint32_t *dstw = reinterpret_cast<uint32_t *>(&S.t);
                    for (uint32_t k = lane; k < sizeof(S.t) / 4; k += 64) dstw[k] = fixed_tabs[k];
                    wave_local_sync();
                    tables = 1;
                }
            } else {
                uint32_t hlit = br_take(hb, 5) + 257u;
                uint32_t hdist = br_take(hb, 5) + 1u;
                uint32_t hclen = br_take(hb, 4) + 4u;
                if (lane < 19) S.lens[lane] = 0;
                wave_local_sync();
                read_cl_lens(S, hb, org, hclen);
                wave_local_sync();
                if (lane < 19) S.cl_len[lane] = S.lens[lane];
                tables = 2;
                if (!build_code(S, CODE_CL, S.lens, 19, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES))) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                if (need_p2 && lane < 19) {
                    uint32_t l = S.cl_len[lane];
                    uint32_t used = l != 0, code = 1234543u;
                    if (used) {
                        uint32_t rank = 0;
                        for (uint32_t j = 0; j < lane; j++) rank += (S.cl_len[j] == l);
                        code = (uint32_t)S.t.first[CODE_CL][l] + rank;
                    }
                    S.cl_code[lane] = code;
                    S.cl_used[lane] = used;
                }
                wave_local_sync();
                const uint32_t total = hlit + hdist;
                const int bad = decode_code_lengths(S, hb, org, total);
                if (bad) { status = DEBIG_E_NO_CODE; break; }
                wave_local_sync();
                if (!build_code(S, CODE_LIT, S.lens, hlit, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES))) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                if (!build_code(S, CODE_DIST, S.lens + hlit, hdist, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES))) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
            }
            if (need_p2) {
                if (row_cur >= slot.rows) { status = DEBIG_E_RETRY; break; }
                if (!fixed && lane < 19) {
                    uint32_t *rw = myrows + (size_t)row_cur * 64u;
                    rw[3 * lane] = S.cl_code[lane];
                    rw[3 * lane + 1] = S.cl_used[lane];
                    rw[3 * lane + 2] = S.cl_len[lane];
                }
                ST_EMIT(REC_P2, row_cur, (uint32_t)fixed, 0u, outpos, 0ull);
                if (status != DEBIG_OK) break;
                row_cur++;
            }
            bitpos = hb.pos;
            const int64_t block_start_bit = bitpos;
            PROF_END(3);
            wave_local_sync(); /* the header scratch becomes the rings */
            staged_valid = 0;

            // ---- symbol windows
            int block_done = 0;
            while (!block_done && status == DEBIG_OK) {
                n_windows++;
                // window origin: the 16-byte aligned address at or below the window's first byte
                const int64_t wb0 = bitpos >> 3;
                const int64_t worg = wb0 - (int64_t)((uintptr_t)(in + wb0) & 15u);
                const uint32_t ws = (uint32_t)(bitpos - 8 * worg); /* window-relative position of the first symbol */
                // strand length: the size of the Huffman block before this one over 64 lanes; no block seen
                // yet: all that is left of the input (a fixed-Huffman stream is rarely more than one block)
                // or ST_DYN_FIRST_GUESS
                const uint64_t rem = (uint64_t)wb0 < in_len ? in_len - (uint64_t)wb0 : 0u;
                const uint64_t guess = blk_guess ? (uint64_t)blk_guess : (fixed ? rem + 16u : (uint64_t)ST_DYN_FIRST_GUESS);
                const uint64_t want = rem + 16u < guess ? rem + 16u : guess;
                uint32_t seg = (uint32_t)(((want + 63u) / 64u + 15u) & ~(uint64_t)15u);
                seg = seg < ST_SEG_MIN ? ST_SEG_MIN : (seg > ST_SEG_MAX ? ST_SEG_MAX : seg);
                const uint32_t segb = 8u * seg;
                // unit rows hold the lanes that have input: 4 lanes (256 bytes) per workspace row
                const uint64_t wlanes = (rem + 16u + (ws >> 3)) / seg + 2u;
                const uint32_t pitch = wlanes >= 64u ? ST_UNIT_ROWS : (uint32_t)((wlanes + 3u) / 4u);
                const int stores = lane < 4u * pitch;
                if (row_cur + ST_INFO_ROWS + pitch > slot.rows) { status = DEBIG_E_RETRY; break; }
                const uint32_t info_row = row_cur;
                const uint32_t unit_row0 = row_cur + ST_INFO_ROWS;

                StLane a;
                uint32_t t[16];
                StTerm TA, TB, TR;
                st_term_clear(TA); st_term_clear(TB); st_term_clear(TR);
                uint32_t dummy_sync = 0;
                uint32_t n_main = 0; /* main unit rows written */
                uint32_t n_patch = 0; /* patch unit rows written */
                // per-lane outcome of the window
                uint32_t seg_nbytes = 0, seg_units = 0, seg_j = 0, seg_npu = 0, seg_adj = 0;
                uint32_t eff_ts = 0; /* the lane's real terminal event */
                int64_t eff_tend_w = 0, end_w = 0; /* window relative */
                int done_window = 0;
                uint32_t last = 0;

                if (short_mode) {
                    // ---- probe: the block before ended inside lane 0's first units; lane 0 alone, from the
                    // true position, looks ST_PROBE_UNITS units far for the end of this one
                    PROF_BEGIN();
                    st_ring_init(rg, in, in_len, bitpos, a, lane == 0);
                    a.nbytes = 0;
                    wave_local_sync();
                    const uint32_t gate = st_gate(in_len, a.org);
                    uint32_t pu = 0;
                    int hit = 0;
                    n_rounds++; /* (debig_result.n_rounds: decode passes -- probe, main pass, every re-decode round) */
                    for (; pu < ST_PROBE_UNITS; pu++) {
                        if (unit_row0 + (pu + 1u) * pitch > slot.rows) break;
                        const uint32_t rb = st_ring_bound(a);
                        a.bound = lane == 0 && TR.ts == 0 ? (gate < rb ? gate : rb) : 0u;
                        st_ring_fetch(in, in_len, a, lane == 0);
                        st_phase<true>(S, rg, a, TR, TB, pu, 0xffffffffu, dummy_sync, t);
                        st_ring_commit(rg, a, lane == 0);
                        if (lane == 0) st_store_unit(myrows + (size_t)(unit_row0 + pu * pitch) * 64u, t);
                        if (lane == 0 && TR.ts == 0 && a.lp >= gate) { /* the tail gate stopped the lane */
                            TR.ts = FL_TAIL; TR.tend = a.lp; TR.fznb = a.nbytes; TR.at = pu;
                        }
                        hit = wave_bcast_u32(TR.ts, 0) != 0;
                        if (hit) { pu++; break; }
                    }
                    PROF_END(1);
                    if (hit) {
                        done_window = 1;
                        last = 0;
                        n_main = pu;
                        seg_nbytes = TR.fznb; seg_units = pu; seg_j = 0; seg_npu = 0; seg_adj = 0;
                        eff_ts = TR.ts;
                        eff_tend_w = (int64_t)TR.tend + 8 * (a.org - worg);
                    } else {
                        short_mode = 0;
                        st_term_clear(TR);
                    }
                    wave_local_sync();
                }
                if (!done_window) {
                    // ---- lead: lanes 1..63 chase positions from ST_LEAD_BITS before their strand.  The lead also COUNTS
                    // its symbols: the symbol density at 63 places of the window.  A stream starts with an empty history,
                    // so its first strands hold twice the symbols of its last ones (64 KiB of text in 64 equal strands: 38
                    // units in lane 0, 16 from lane 30 on: the main pass lasts 38 phases where 20 would do).  When the
                    // estimated symbols per strand differ enough the strands are CUT AGAIN, at equal shares of the
                    // estimated symbols, and the lead runs once more from the new places (three cheap phases).
                    PROF_BEGIN();
                    int64_t lo_w = (int64_t)lane * segb, hi_w = lo_w + segb;
                    const uint32_t lead_bits = segb >= ST_REBALANCE_MIN_BITS ? ST_LEAD_BITS_LONG : ST_LEAD_BITS;
                    const uint32_t lm_lead = S.t.mask[CODE_LIT], dm_lead = S.t.mask[CODE_DIST];
                    for (uint32_t pass = 0; pass < 2u; pass++) {
                        const int64_t start_w0 = lane == 0 ? (int64_t)ws : lo_w - (int64_t)lead_bits;
                        if (pass) wave_local_sync();
                        st_ring_init(rg, in, in_len, 8 * worg + start_w0, a, 1);
                        a.nbytes = 0;
                        wave_local_sync();
                        const uint32_t lo_rel = st_rel(lo_w, worg, a.org);
                        uint32_t nlead = 0;
                        for (uint32_t it = 0; it < 4096u; it++) {
                            const uint32_t rb = st_ring_bound(a);
                            a.bound = lane == 0 ? 0u : (lo_rel < rb ? lo_rel : rb);
                            if (!__any(lane != 0 && a.lp < lo_rel)) break;
                            st_ring_fetch(in, in_len, a, lane != 0 && a.lp < lo_rel);
ST_NOUNROLL
                            for (uint32_t k = 0; k < ST_UNIT_TOK; k += 3u) {
                                st_step_lead(S, rg, a, lm_lead, dm_lead, nlead);
                                st_step_lead(S, rg, a, lm_lead, dm_lead, nlead);
                                st_step_lead(S, rg, a, lm_lead, dm_lead, nlead);
                            }
                            st_ring_commit(rg, a, 1);
                        }
                        if (pass || !ST_REBALANCE || segb < ST_REBALANCE_MIN_BITS) break;
                        // estimated symbols of strand L: its length x the mean of the densities at its two ends
                        // (a lead is two dozen symbols: the counts are smoothed over five neighbours -- the trend is what
                        // matters -- and lane 0, which has no lead, continues the slope of its neighbours)
                        uint32_t dl;
                        {
                            const uint32_t c1 = (uint32_t)__shfl((int)nlead, 1);
                            const uint32_t raw = lane == 0 ? c1 : nlead;
                            const uint32_t m1 = (uint32_t)__shfl_up((int)raw, 1), m2 = (uint32_t)__shfl_up((int)raw, 2);
                            const uint32_t p1 = (uint32_t)__shfl_down((int)raw, 1), p2 = (uint32_t)__shfl_down((int)raw, 2);
                            const uint32_t a1 = lane >= 1u ? m1 : raw, a2 = lane >= 2u ? m2 : a1;
                            const uint32_t b1 = lane <= 62u ? p1 : raw, b2 = lane <= 61u ? p2 : b1;
                            const uint32_t sm = a2 + 2u * a1 + 3u * raw + 2u * b1 + b2; /* x 9 */
                            const uint32_t s2 = (uint32_t)__shfl((int)sm, 2), s4 = (uint32_t)__shfl((int)sm, 4);
                            const uint32_t s1 = (uint32_t)__shfl((int)sm, 1);
                            // lanes 0 and 1 sit on the steep end: extrapolate the slope between lanes 2 and 4
                            const uint32_t slope = s2 > s4 ? (s2 - s4) / 2u : 0u;
                            dl = lane == 0 ? s2 + 2u * slope : lane == 1u ? (s1 > s2 + slope ? s1 : s2 + slope) : sm;
                        }
#ifndef ST_REBALANCE_GAIN_X4
#define ST_REBALANCE_GAIN_X4 5 /* contrast gain x 4: a lead decodes from a guess, and until it falls into step its symbols have
                                  the lengths of garbage, not of the data around it: the measured densities understate the
                                  trend (text: 1.8 : 1 measured where the strands' symbol counts are 2.4 : 1) */
#endif
                        {
                            uint32_t dsum;
                            (void)wave_excl_scan_u32(dl, &dsum);
                            const int32_t mean = (int32_t)(dsum >> 6);
                            const int32_t amp = mean + (((int32_t)dl - mean) * (int32_t)ST_REBALANCE_GAIN_X4) / 4;
                            dl = (uint32_t)(amp < mean / 4 + 1 ? mean / 4 + 1 : amp);
                        }
                        const uint32_t dl_next = (uint32_t)__shfl_down((int)dl, 1); /* (collectives stay outside of ?: every lane takes part) */
                        const uint32_t dr = lane == 63u ? dl : dl_next;
                        const uint32_t est = (segb >> 6) * (dl + dr);                 /* < 2^24 (the counts are x 9) */
                        uint32_t tot;
                        const uint32_t pre = wave_excl_scan_u32(est, &tot);
                        const uint32_t mx = wave_max_u32(est);
                        if ((uint64_t)mx * 64u * 8u <= (uint64_t)tot * 9u) break;     /* the densest strand is within 1/8 of the mean */
                        // boundary k at k / 64 of the estimated symbols: inside strand j, linearly
                        const uint32_t tk = (uint32_t)(((uint64_t)tot * lane) >> 6);
                        uint32_t j = 0;
DEV_UNROLL
                        for (uint32_t step = 32; step; step >>= 1) {
                            const uint32_t c = j + step;
                            const uint32_t pc = (uint32_t)__shfl((int)pre, (int)(c & 63u));
                            if (c < 64u && pc <= tk) j = c;
                        }
                        const uint32_t pj = (uint32_t)__shfl((int)pre, (int)j), ej = (uint32_t)__shfl((int)est, (int)j);
                        const float fr = ej ? (float)(tk - pj) / (float)ej : 0.0f;
                        uint32_t nb = j * segb + (uint32_t)((float)segb * fr);
                        nb = lane == 0 ? 0u : (nb & ~7u);
                        const uint32_t nb_next = (uint32_t)__shfl_down((int)nb, 1);
                        const uint32_t nxt = lane == 63u ? 64u * segb : nb_next;
                        const uint32_t gap = nxt - nb;
                        // every strand must hold its lead and stay within what a unit header can address
                        if (__any(nxt <= nb || gap < lead_bits + 256u || gap > 8u * ST_STRAND_MAX)) break;
                        lo_w = (int64_t)nb;
                        hi_w = (int64_t)nxt;
                    }
                    PROF_END(1);
                    // ---- main pass
                    PROF_BEGIN();
                    uint32_t start_w = (uint32_t)((int64_t)a.lp + 8 * (a.org - worg)); /* where my decode of the strand began */
                    const uint32_t hi_rel = st_rel(hi_w, worg, a.org);
                    const uint32_t gate = st_gate(in_len, a.org);
                    const uint32_t lim = hi_rel < gate ? hi_rel : gate;
                    uint32_t cK = 0xffffffffu, nbK = 0; /* where unit ST_SYNC_UNIT of this decode began (lane relative) */
                    uint32_t nu = 0;                    /* units in which the lane was still going */
                    uint32_t u = 0;
                    n_rounds++;
                    uint32_t kcut = 63; /* 0 once lane 0 -- which decodes from the true position -- has met the block's
                                           terminal event: nothing behind its strand counts.  (A terminal event of any
                                           other lane proves nothing before the lanes in front of it have finished, and
                                           those finish when everybody does: guessing lanes meet such events all the time.) */
                    for (;; u++) {
                        const int going = a.lp < lim && !(lane == 0 && TA.ts != 0);
                        if (wave_bcast_u32(TA.ts, 0) != 0) kcut = 0;
                        if (!__any(going && lane <= kcut)) break;
                        if (unit_row0 + (u + 1u) * pitch > slot.rows) { status = DEBIG_E_RETRY; break; }
                        if (u == ST_SYNC_UNIT) {
                            st_term_clear(TB);
                            if (going) { cK = a.lp; nbK = a.nbytes; }
                        }
                        const uint32_t rb = st_ring_bound(a);
                        a.bound = lim < rb ? lim : rb;
                        st_ring_fetch(in, in_len, a, going);
                        st_phase<false>(S, rg, a, TA, TB, u, 0xffffffffu, dummy_sync, t);
                        st_ring_commit(rg, a, going); /* the wait for the loads comes before the unit's stores are issued */
                        if (stores) st_store_unit(myrows + (size_t)(unit_row0 + u * pitch) * 64u + 16u * lane, t);
                        nu += (uint32_t)going;
                    }
                    if (status != DEBIG_OK) break;
                    if (wave_bcast_u32(TA.ts, 0) != 0) kcut = 0;
                    n_main = u;
                    PROF_END(2);
                    PROF_BEGIN();
                    // the tail gate: a lane that stopped in front of its strand's end
                    if (a.lp < hi_rel && a.lp >= gate) {
                        if (TA.ts == 0) { TA.ts = FL_TAIL; TA.tend = a.lp; TA.fznb = a.nbytes; TA.at = nu ? nu - 1u : 0u; }
                        if (TB.ts == 0) { TB.ts = FL_TAIL; TB.tend = a.lp; TB.fznb = a.nbytes; TB.at = nu ? nu - 1u : 0u; }
                    }
                    // first-decode results, window relative
                    const int64_t lorg = 8 * (a.org - worg);
                    end_w = (int64_t)a.lp + lorg;
                    const int64_t end1_w = end_w; /* where the first decode ended: what holds again once a re-decode has joined it */
                    const uint32_t cK_w = cK == 0xffffffffu ? 0xffffffffu : (uint32_t)((int64_t)cK + lorg);
                    const uint32_t nb_fin = a.nbytes;
                    // outcome if the lane was right from the start
                    uint32_t mode = 0; /* 0 first decode as it is, 1 patch + first decode from ST_SYNC_UNIT, 2 patch only */
                    eff_ts = TA.ts;
                    eff_tend_w = (int64_t)TA.tend + lorg;
                    seg_nbytes = TA.ts ? TA.fznb : nb_fin;
                    seg_units = TA.ts ? umin32((TA.at & 0xffffu) + 1u, nu) : nu; /* (the tail gate can stop a lane before its first unit) */
                    seg_j = 0; seg_npu = 0; seg_adj = 0;
                    // ---- chain: a lane must have started where the lane before it ended
                    for (uint32_t round = 0; round < 66u; round++) {
                        const uint32_t prev_end = (uint32_t)__shfl_up((uint32_t)end_w, 1);
                        const int mismatch = lane > 0 && start_w != prev_end;
                        // the window ends with the first lane that met a terminal event AND started where the lane
                        // before it ended: a guessing lane's events prove nothing (it meets them in garbage all the
                        // time), and lanes behind the block's real end are not worth decoding again
                        const unsigned long long tm = __ballot(eff_ts != 0 && !mismatch);
                        last = tm ? (uint32_t)(__ffsll(tm) - 1) : 63u;
                        last = last < kcut ? last : kcut;
                        const int need = mismatch && lane <= last;
                        if (!__any(need)) break;
                        // decode those lanes again from where the lane before them ended: strictly (a terminal
                        // event stops the lane) and only until they reach the start of unit ST_SYNC_UNIT of
                        // their first decode
                        wave_local_sync();
                        StLane b;
                        st_ring_init(rg, in, in_len, 8 * worg + (int64_t)prev_end, b, need);
                        b.nbytes = 0;
                        wave_local_sync();
                        const int64_t blorg = 8 * (b.org - worg);
                        const uint32_t bhi = st_rel(hi_w, worg, b.org), bgate = st_gate(in_len, b.org);
                        const uint32_t blim = bhi < bgate ? bhi : bgate;
                        const uint32_t sync_at = (need && cK_w != 0xffffffffu && (int64_t)cK_w >= blorg) ? (uint32_t)((int64_t)cK_w - blorg) : 0xffffffffu;
                        uint32_t synced = 0;
                        st_term_clear(TR);
                        uint32_t pu = 0, mypu = 0;
                        n_rounds++;
                        const uint32_t patch_row0 = unit_row0 + n_main * pitch;
                        for (;; pu++) {
                            const int going = need && !synced && TR.ts == 0 && b.lp < blim;
                            if (!__any(going)) break;
                            if (patch_row0 + (pu + 1u) * pitch > slot.rows) { status = DEBIG_E_RETRY; break; }
                            const uint32_t rb = st_ring_bound(b);
                            b.bound = going ? (blim < rb ? blim : rb) : 0u;
                            st_ring_fetch(in, in_len, b, going);
                            st_phase<true>(S, rg, b, TR, TB, pu, sync_at, synced, t);
                            st_ring_commit(rg, b, going);
                            if (going && stores) st_store_unit(myrows + (size_t)(patch_row0 + pu * pitch) * 64u + 16u * lane, t);
                            if (going && !synced && TR.ts == 0 && b.lp == sync_at) synced = 1u; /* exactly between two phases */
                            mypu += (uint32_t)going;
                        }
                        if (status != DEBIG_OK) break;
                        n_patch = pu > n_patch ? pu : n_patch;
                        if (need) {
                            // a lane that stops exactly at the sync position between two phases
                            if (!synced && TR.ts == 0 && b.lp == sync_at) synced = 1u;
                            start_w = prev_end;
                            seg_npu = mypu;
                            if (synced) {
                                mode = 1;
                                end_w = end1_w; /* (an earlier round may have decoded this lane to its end from a wrong start) */
                                seg_j = ST_SYNC_UNIT;
                                seg_adj = b.nbytes - nbK;
                                eff_ts = TB.ts;
                                eff_tend_w = (int64_t)TB.tend + lorg;
                                seg_nbytes = b.nbytes + ((TB.ts ? TB.fznb : nb_fin) - nbK);
                                seg_units = TB.ts ? umin32((TB.at & 0xffffu) + 1u, nu) : nu;
                                if (seg_units < ST_SYNC_UNIT) seg_units = ST_SYNC_UNIT; /* (not reached: TB is armed from that unit on) */
                            } else {
                                mode = 2;
                                if (TR.ts == 0 && b.lp < bhi && b.lp >= bgate) { TR.ts = FL_TAIL; TR.tend = b.lp; TR.fznb = b.nbytes; }
                                seg_j = 0; seg_units = 0; seg_adj = 0;
                                eff_ts = TR.ts;
                                eff_tend_w = (int64_t)TR.tend + blorg;
                                seg_nbytes = TR.ts ? TR.fznb : b.nbytes;
                                end_w = (int64_t)b.lp + blorg;
                            }
                        }
                    }
                    if (status != DEBIG_OK) break;
                    (void)mode;
                    PROF_END(4);
                    wave_local_sync();
                }
                // ---- the window's verdict and its records
                PROF_BEGIN();
                const int used = lane <= last;
                const uint32_t wts = wave_bcast_u32(eff_ts, last);
                const uint32_t wflag = wts & 0xffu, wstatus = wts >> 8;
                const uint32_t wt_lo = wave_bcast_u32((uint32_t)eff_tend_w, last), wt_hi = wave_bcast_u32((uint32_t)((uint64_t)eff_tend_w >> 32), last);
                const uint32_t we_lo = wave_bcast_u32((uint32_t)end_w, last), we_hi = wave_bcast_u32((uint32_t)((uint64_t)end_w >> 32), last);
                const int64_t tend_last = (int64_t)(((uint64_t)wt_hi << 32) | wt_lo), end_last = (int64_t)(((uint64_t)we_hi << 32) | we_lo);
                const int64_t wend = 8 * worg + (wflag != FL_CONT ? tend_last : end_last);
                const uint32_t nbytes = used ? seg_nbytes : 0u;
                uint32_t wtotal;
                (void)wave_excl_scan_u32(nbytes, &wtotal);
                {
                    uint32_t *ir = myrows + (size_t)info_row * 64u;
                    ir[lane] = nbytes;
                    ir[64u + lane] = used ? (seg_units | (seg_j << 10) | (seg_npu << 20)) : 0u;
                    ir[128u + lane] = seg_adj;
                    ir[192u + lane] = 0u;
                }
                ST_EMIT(REC_WIN2, info_row, (last + 1u) | (wflag << 8), wstatus, (uint64_t)wtotal,
                        (uint64_t)n_main | ((uint64_t)n_patch << 20) | ((uint64_t)pitch << 40));
                if (status != DEBIG_OK) break;
                row_cur = unit_row0 + (n_main + n_patch) * pitch;
                outpos += wtotal;
                bitpos = wend;
                short_mode = last == 0 && wflag != FL_CONT && wave_bcast_u32(seg_units, 0) <= ST_PROBE_UNITS;
                PROF_END(4);
                if (wflag == FL_EOB) block_done = 1;
                else if (wflag == FL_TAIL) { block_done = 1; more = 0; }
                else if (wflag == FL_ERR) { status = wstatus; }
            }
            if (status == DEBIG_OK) {
                // the next block is probably about as long as this one (+ 1/8: a block that does not fit
                // one window costs a second, mostly idle one)
                const uint64_t blen = (uint64_t)((bitpos - block_start_bit) >> 3);
                const uint64_t g = blen + (blen >> 3) + 64u;
                blk_guess = g > 0x7fffffffu ? 0x7fffffffu : (uint32_t)g;
            }
            wave_local_sync(); /* the rings become header scratch again */
        }
        end_bits = bitpos;
    }
#undef ST_EMIT
    *state_out = status == DEBIG_E_RETRY ? (uint32_t)DEBIG_E_RETRY : (uint32_t)DEBIG_OK;
    if (lane == 0) {
        debig_ws_rec rr;
        rr.kind = REC_END;
        rr.row = final_set;
        rr.a = status;
        rr.b = n_blocks;
        rr.c = (uint64_t)end_bits;
        rr.d = (uint64_t)n_windows | ((uint64_t)n_rounds << 32);
        myrec[rec_cur < slot.recs ? rec_cur : slot.recs - 1u] = rr;
        slots[sid].state = status == DEBIG_E_RETRY ? (uint32_t)DEBIG_E_RETRY : (uint32_t)DEBIG_OK;
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
        PROF_STORE(results[sid]);
#endif
    }
    (void)results;
}

// ------------------------------------------------------------------ LZ77 half: a strand window
// REC_WIN2 of lz_body: the window's units in stream order (segment by segment: patch units, then the
// first decode's units from the segment's sync unit on), 64 at a time, one per lane.  A unit knows
// where its output starts (header) and holds its 15 tokens in four 16-byte loads: the placement is
// straight-line code over registers; as many consecutive units as fit the tile in one piece make a
// batch, then the far / near machinery of the 68-byte path takes over.
template <class LDS>
DEV_INLINE void lz_replay_units(LDS &S, OutState &O, const debig_ws_rec &rec, const uint32_t *myrows, uint32_t &status LZ_PROF_PARAM)
{
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
    uint64_t prof_t0 = 0;
#endif
    const uint32_t lane = lane_id();
    const uint32_t used_n = rec.a & 0xffu;
    const uint32_t *ir = myrows + (size_t)rec.row * 64u;
    const uint32_t nbytes = lane < used_n ? ir[lane] : 0u;
    const uint32_t pk = lane < used_n ? ir[64u + lane] : 0u;
    const uint32_t adj = lane < used_n ? ir[128u + lane] : 0u;
    const uint32_t nu = pk & 1023u, sj = (pk >> 10) & 1023u, npu = pk >> 20;
    const uint32_t m = npu + (nu > sj ? nu - sj : 0u);
    uint32_t wtotal, mtot;
    const uint32_t pre = wave_excl_scan_u32(nbytes, &wtotal);
    const uint32_t mex = wave_excl_scan_u32(m, &mtot);
    const uint32_t n_main = (uint32_t)rec.d & 0xfffffu, pitch = (uint32_t)(rec.d >> 40);
    const uint32_t *ubase = myrows + (size_t)(rec.row + ST_INFO_ROWS) * 64u;
    const int64_t w_out0 = O.outpos;
    const uint64_t cap_left = O.out_cap > (uint64_t)w_out0 ? O.out_cap - (uint64_t)w_out0 : 0u;
    const uint32_t cap_w = cap_left > 0x7fffffffu ? 0x7fffffffu : (uint32_t)cap_left; /* recipient bytes from w_out0 */
#ifndef ST_REPLAY_TWO_ROUNDS
#define ST_REPLAY_TWO_ROUNDS 0 /* the units of a tile's first two rounds asked for together: within noise (4096 x 64 KiB: 0.898 vs
                                 0.888 ms, 2048: 0.610 vs 0.617; profiles/r04_strand_notes.txt): the unit loads are not what
                                 the replay waits for */
#endif
    // the unit with stream index g0 + lane: its 16 words and where its output starts / ends (window relative)
#define ST_FETCH_UNITS(G0, W, USTART, UEND)                                                                         \
    do {                                                                                                            \
        const uint32_t g_ = (G0) + lane;                                                                            \
        const int has_ = g_ < mtot;                                                                                 \
        uint32_t L_ = 0; /* the segment of unit g: the last lane whose first unit is at or before g */             \
        DEV_UNROLL                                                                                                  \
        for (uint32_t step_ = 32; step_; step_ >>= 1) {                                                             \
            const uint32_t c_ = L_ + step_;                                                                         \
            const uint32_t mc_ = (uint32_t)__shfl((int)mex, (int)(c_ & 63u));                                       \
            if (c_ < 64u && mc_ <= g_) L_ = c_;                                                                     \
        }                                                                                                           \
        const uint32_t r_ = g_ - (uint32_t)__shfl((int)mex, (int)L_);                                               \
        const uint32_t npuL_ = (uint32_t)__shfl((int)npu, (int)L_), sjL_ = (uint32_t)__shfl((int)sj, (int)L_);     \
        const uint32_t preL_ = (uint32_t)__shfl((int)pre, (int)L_), adjL_ = (uint32_t)__shfl((int)adj, (int)L_);   \
        const int ispatch_ = r_ < npuL_;                                                                            \
        const uint32_t urow_ = ispatch_ ? n_main + r_ : sjL_ + (r_ - npuL_);                                        \
        if (has_) {                                                                                                 \
            const uint32_t *up_ = ubase + (size_t)urow_ * pitch * 64u + L_ * 16u;                                   \
            st_load_unit16(up_, W[0], W[1], W[2], W[3]);                                                            \
            st_load_unit16(up_ + 4, W[4], W[5], W[6], W[7]);                                                        \
            st_load_unit16(up_ + 8, W[8], W[9], W[10], W[11]);                                                      \
            st_load_unit16(up_ + 12, W[12], W[13], W[14], W[15]);                                                   \
        } else {                                                                                                    \
            DEV_UNROLL                                                                                              \
            for (uint32_t k_ = 0; k_ < 16; k_++) W[k_] = k_ < 15u ? TOK_NOP : 0u;                                   \
        }                                                                                                           \
        USTART = has_ ? preL_ + (ispatch_ ? 0u : adjL_) : wtotal; /* + the header's offset field, once loaded */    \
        UEND = has_ ? 1u : 0u;                                                                                      \
    } while (0)

    // one round: the (at most 64) units in W -- one per lane -- that still fit the tile are placed.  NFIT: how many
    // (0: the tile is full).  Straight-line code over registers: 15 tokens per lane, literals and match descriptors into
    // the tile, a bit per match into the far / near map.
#define ST_PLACE_ROUND(W, UBASE, UHAS, NFIT)                                                                          \
    do {                                                                                                              \
        const uint32_t ustart_ = (UHAS) ? (UBASE) + (W[15] & 0xfffffu) : wtotal; /* window relative */                \
        const uint32_t uend_ = ustart_ + (W[15] >> 20);                                                               \
        {                                                                                                             \
            const int fit_ = (UHAS) && uend_ - b_rel0 <= room_tile;                                                   \
            const unsigned long long fm_ = __ballot(fit_);                                                            \
            NFIT = ~fm_ == 0ull ? 64u : (uint32_t)(__ffsll(~fm_) - 1);                                                \
        }                                                                                                             \
        if (wave_bcast_u32(ustart_, 0) != e_last) { /* (units follow each other: not reached) */                      \
            status = DEBIG_E_INTERNAL;                                                                                \
            any_err = 1;                                                                                              \
            NFIT = 0;                                                                                                 \
        }                                                                                                             \
        if (NFIT != 0) {                                                                                              \
            e_last = wave_bcast_u32(uend_, NFIT - 1u);                                                                \
            const int chk_cap_ = e_last > cap_w; /* the recipient ends inside this round */                           \
            if (lane < NFIT) {                                                                                        \
                uint32_t rel_ = (uint32_t)(w_out0 - O.tile_base) + ustart_;                                           \
                if (!chk_far && !chk_cap_) { /* (wave-uniform) the usual round: nothing can fail here */              \
                    DEV_UNROLL                                                                                        \
                    for (uint32_t k_ = 0; k_ < ST_UNIT_TOK; k_++) {                                                   \
                        const uint32_t tk_ = W[k_];                                                                   \
                        const uint32_t is_len_ = tk_ >> 31, nop_ = (tk_ >> 30) & 1u, len3_ = (tk_ >> 16) & 0xffu;     \
                        if (!nop_) {                                                                                  \
                            S.tile[rel_] = (typename LDS::Elem)(is_len_ ? len3_ : tk_);                               \
                            if (is_len_) {                                                                            \
                                const uint32_t dm1_ = tk_ & 0x7fffu;                                                  \
                                S.tile[rel_ + 1] = (typename LDS::Elem)(dm1_ & 255u);                                 \
                                S.tile[rel_ + 2] = (typename LDS::Elem)(dm1_ >> 8);                                   \
                                uint32_t *map_ = ((int32_t)(rel_ + len3_ + 3u) - (int32_t)(dm1_ + 1u) <= (int32_t)lds_rel) ? S.farmap : S.bitmap; \
                                atomicOr(&map_[rel_ >> 5], 1u << (rel_ & 31u));                                       \
                            }                                                                                         \
                        }                                                                                             \
                        rel_ += is_len_ ? len3_ + 3u : (nop_ ^ 1u);                                                   \
                    }                                                                                                 \
                } else {                                                                                              \
                    DEV_UNROLL                                                                                        \
                    for (uint32_t k_ = 0; k_ < ST_UNIT_TOK; k_++) {                                                   \
                        const uint32_t tk_ = W[k_];                                                                   \
                        const uint32_t is_len_ = tk_ >> 31, nop_ = (tk_ >> 30) & 1u, len3_ = (tk_ >> 16) & 0xffu;     \
                        const uint32_t outlen_ = is_len_ ? len3_ + 3u : (nop_ ^ 1u);                                  \
                        const uint32_t dm1_ = tk_ & 0x7fffu;                                                          \
                        /* src/inflate.c:1843: distance beyond the start of the output | the output would exceed recipient_size */ \
                        const int too_far_ = chk_far && is_len_ && (int32_t)(dm1_ + 1u) > tb32 + (int32_t)rel_;       \
                        const int full_ = chk_cap_ && rel_ + outlen_ > cap_rel;                                       \
                        if ((too_far_ || full_) && err_pos == 0xffffffffu) {                                          \
                            err_pos = rel_;                                                                           \
                            err_st = too_far_ ? (uint32_t)DEBIG_E_DIST_TOO_FAR : (uint32_t)DEBIG_E_OUTPUT_FULL;       \
                        }                                                                                             \
                        if (err_pos == 0xffffffffu && !nop_) {                                                        \
                            S.tile[rel_] = (typename LDS::Elem)(is_len_ ? len3_ : tk_);                               \
                            if (is_len_) {                                                                            \
                                S.tile[rel_ + 1] = (typename LDS::Elem)(dm1_ & 255u);                                 \
                                S.tile[rel_ + 2] = (typename LDS::Elem)(dm1_ >> 8);                                   \
                                uint32_t *map_ = ((int32_t)(rel_ + len3_ + 3u) - (int32_t)(dm1_ + 1u) <= (int32_t)lds_rel) ? S.farmap : S.bitmap; \
                                atomicOr(&map_[rel_ >> 5], 1u << (rel_ & 31u));                                       \
                            }                                                                                         \
                        }                                                                                             \
                        rel_ += outlen_;                                                                              \
                    }                                                                                                 \
                }                                                                                                     \
            }                                                                                                         \
            g0 += NFIT;                                                                                               \
            if ((chk_far || chk_cap_) && __any(err_pos != 0xffffffffu)) any_err = 1;                                  \
        }                                                                                                             \
    } while (0)

    for (uint32_t g0 = 0; g0 < mtot && status == DEBIG_OK;) {
        // ---- one tile of output: rounds of up to 64 units (one per lane) are placed until the tile is full, then
        // the matches of the whole tile are resolved.  (A round of 64 units is as little as 1 KB of literal-heavy
        // data: the far / near passes -- barriers, span scans -- must not be paid per round.)
        PROF_BEGIN();
        // the tile restarts at this batch's first byte; its stores stay in flight until the fence before the far copy
        if (O.outpos > O.lds_from) lz_flush_all(S, O, 0);
        const uint32_t b_rel0 = (uint32_t)(O.outpos - w_out0);
        const int32_t tb32 = O.tile_base > 70000 ? 70000 : (int32_t)O.tile_base;
        const int chk_far = tb32 < 32768; /* a distance can only be too far near the start */
        const int64_t room = (int64_t)O.out_cap - O.tile_base;
        const uint32_t cap_rel = room > 0x7fffffff ? 0x7fffffffu : (room < 0 ? 0u : (uint32_t)room);
        const uint32_t lds_rel = (uint32_t)(O.lds_from - O.tile_base);
        const uint32_t room_tile = (uint32_t)LDS::T2 - 16u; /* output bytes of this batch (tile_base is at most 15 below its first byte) */
        uint32_t e_last = b_rel0;
        uint32_t err_pos = 0xffffffffu, err_st = 0;
        int any_err = 0;
        {
            uint32_t wa[16], wb[16], ba, bb, ha, hb = 0, nfit = 0;
            const uint32_t g_first = g0;
            const int two = ST_REPLAY_TWO_ROUNDS && g_first + 64u < mtot;
            ST_FETCH_UNITS(g_first, wa, ba, ha);
            if (two) ST_FETCH_UNITS(g_first + 64u, wb, bb, hb);
            ST_PLACE_ROUND(wa, ba, ha, nfit);
            if (nfit == 0 && !any_err) { status = DEBIG_E_INTERNAL; any_err = 1; } /* (a unit is at most 3870 bytes: not reached) */
            if (two && nfit == 64u && !any_err) ST_PLACE_ROUND(wb, bb, hb, nfit);
            while (nfit == 64u && g0 < mtot && !any_err) { /* literal-heavy data: more rounds fit */
                ST_FETCH_UNITS(g0, wa, ba, ha);
                ST_PLACE_ROUND(wa, ba, ha, nfit);
            }
        }
        if (status != DEBIG_OK) break;
        int64_t w_out1 = w_out0 + (int64_t)e_last;
        if (any_err) {
            const uint32_t ep = wave_min_u32(err_pos); /* the output ends at the first failing token */
            const unsigned long long em = __ballot(err_pos == ep);
            status = wave_bcast_u32(err_st, (uint32_t)(__ffsll(em) - 1));
            w_out1 = O.tile_base + (int64_t)ep;
        }
        const uint32_t from_rel = (uint32_t)(O.outpos - O.tile_base);
        const uint32_t to_rel = (uint32_t)(w_out1 - O.tile_base);
        PROF_END(0);
        PROF_BEGIN();
        wave_mem_fence(); /* the flushed tile is history now */
        lz_publish(O);
        wave_local_sync();
#if !(defined(DEBIG_ABLATE) && (DEBIG_ABLATE & 1)) /* timing experiment: far copy skipped (wrong output) */
        far_copy_u(S, O, from_rel, to_rel);
#endif
        PROF_END(1);
        PROF_BEGIN();
#if !(defined(DEBIG_ABLATE) && (DEBIG_ABLATE & 2)) /* timing experiment: near resolve skipped (wrong output) */
        resolve_matches_groups_u(S, O, from_rel, to_rel);
#endif
        PROF_END(2);
        if (status != DEBIG_OK) { /* drop the marks of matches at or beyond the failing position */
            for (uint32_t k = lane; k < LDS::MAP_WORDS; k += 64) { S.bitmap[k] = 0; S.farmap[k] = 0; }
            wave_local_sync();
        }
        O.outpos = w_out1;
    }
#undef ST_PLACE_ROUND
#undef ST_FETCH_UNITS
}

// ---- scan and LZ77 halves in one kernel (debig_scanlz_kernel's shape): the wavefront that scanned a
// stream replays it; LDS is the union of the two layouts
struct __attribute__((aligned(16))) StrandLzLds {
    union {
        StrandLds s;
        LzLds l;
    };
};

__global__ void __launch_bounds__(64) DEBIG_LZ_ATTRS
debig_strand_kernel(const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                    const debig_stream *__restrict__ streams, uint32_t n_streams,
                    const uint32_t *__restrict__ fixed_tabs, debig_ws_slot *__restrict__ slots,
                    debig_ws_rec *__restrict__ recs, uint32_t *__restrict__ rows, debig_result *results)
{
    __shared__ StrandLzLds U;
    if (blockIdx.x >= n_streams) return;
    const uint32_t sid = split_perm(slots, n_streams)[blockIdx.x]; /* the plan kernel's dispatch order */
    const debig_stream st = streams[sid];
    const debig_ws_slot slot = slots[sid];
    uint32_t state = DEBIG_E_RETRY;
    strand_scan_body(U.s, in_arena, out_arena, st, sid, fixed_tabs, slots, recs, rows, results, &state);
    wave_mem_fence(); /* units, records, stored-block copies: in L2 before anything is read back */
    wave_local_sync();
#if !(defined(DEBIG_ABLATE) && (DEBIG_ABLATE & 8)) /* timing experiment: the scan alone (no output) */
    lz_stream(U.l, sid, slot, state, out_arena, streams, results, recs, rows);
#endif
}

// ---- the same two halves as a PIPELINE inside the workgroup: wavefront 0 scans the stream, wavefront 1 replays what
// wavefront 0 has finished, record by record (a window, a stored block).  Few hundred to two thousand streams leave
// most SIMDs with one or two wavefronts, each bound by the latency of its own chain: a stream then takes max(scan,
// LZ77) instead of their sum.  LDS is the SUM of the two layouts (18.8 KB: 8 workgroups per CU); nothing in either
// half is a workgroup barrier (wave_local_sync), the hand-over is a count of complete records in LDS.
template <class LZ> struct __attribute__((aligned(16))) StrandPipeLds {
    StrandLds s;
    LZ l;
    volatile uint32_t produced, done, final_state, pad;
};

// LZ: the LZ77 half's LDS -- LzLds (5 KB tile, 18.8 KB per workgroup: 8 per CU) or LzLdsBig (12 KB tile: 5 per CU, up to
// 1280 streams resident)
template <class LZ>
__global__ void __launch_bounds__(128) DEBIG_LZ_ATTRS
debig_strand_pipe_kernel(const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                         const debig_stream *__restrict__ streams, uint32_t n_streams,
                         const uint32_t *__restrict__ fixed_tabs, debig_ws_slot *__restrict__ slots,
                         debig_ws_rec *__restrict__ recs, uint32_t *__restrict__ rows, debig_result *results)
{
    __shared__ StrandPipeLds<LZ> P;
    if (blockIdx.x >= n_streams) return;
    const uint32_t sid = split_perm(slots, n_streams)[blockIdx.x]; /* the plan kernel's dispatch order */
    if (threadIdx.x == 0) { P.produced = 0; P.done = 0; P.final_state = DEBIG_E_RETRY; }
    __syncthreads(); /* the only workgroup barrier */
    const debig_ws_slot slot = slots[sid];
    if (wave_id() == 0) {
        const debig_stream st = streams[sid];
        uint32_t state = DEBIG_E_RETRY;
        strand_scan_body(P.s, in_arena, out_arena, st, sid, fixed_tabs, slots, recs, rows, results, &state, &P.produced);
        wave_mem_fence(); /* the END record */
        wave_local_sync();
        if (lane_id() == 0) { P.final_state = state; P.done = 1; }
    } else {
        LzPipe pipe;
        pipe.produced = &P.produced;
        pipe.done = &P.done;
        // (a scan that gives the stream up -- workspace share too small -- says so in its END record: the result is
        // DEBIG_E_RETRY as in the other kernels and debig_inflate_kernel takes the stream in the launch that follows)
        lz_stream(P.l, sid, slot, slot.recs == 0 ? (uint32_t)DEBIG_E_RETRY : (uint32_t)DEBIG_OK, out_arena, streams, results, recs, rows, &pipe);
    }
}
