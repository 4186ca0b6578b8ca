// inflate_kernel.inc -- batched DEFLATE inflate for MI355X (gfx950), one wavefront per stream.
//
// Included by debig_hip.hip (hipcc, the product) and by tools/simt_emu/emu_lib.cpp (g++,
// CPU lock-step emulation used only by the CPU test-suite).
//
// What it replaces: reference src/inflate.c:786-1965 (inflate()), observable behaviour
// per SURVEY.md Appendix E, quirks Q1-Q15 included.
//
// Design (MI355X-first, not a translation of the reference's hashed tables):
//
//   * one 64-lane wavefront == one workgroup == one DEFLATE stream at a time.
//   * Huffman tables live in LDS per wavefront: a 2^9 (litlen) / 2^8 (distance) direct
//     table of u32 {length | extra | kind | base} for short codes plus a canonical
//     first/count/offset fallback for codes longer than the table index; built by the whole
//     wavefront (ballot ranks), the fixed code once per process.
//   * TWO PASSES per 4352-byte window of compressed input (staged with 16 B/lane loads):
//       pass 1 (boundary scan, speculative): the window is cut into 64 segments of 68 bytes,
//         one per lane.  Every lane decodes its segment from a guessed bit position; lane
//         L+1 then restarts from the bit position where lane L ended, until the chain of
//         (start == predecessor's end) holds from lane 0 on (Huffman codes self-synchronise:
//         ~3 rounds; worst case it degrades to a serial scan).  The scan is lenient and
//         freezes what a strict decoder would have seen, so valid lanes reproduce the
//         reference exactly.  It yields per segment {bit offset, output count, symbol count}
//         plus the same triple at the middle of the segment.
//       pass 2 (parallel decode): a wavefront prefix sum turns the counts into output
//         offsets; two batches of 64 half-segments are decoded again, literals go to a 4 KiB
//         LDS output tile, each match leaves a 3-byte descriptor + a bitmap bit.
//   * LZ77: matches whose whole source is already flushed have no ordering constraint and are
//     copied first, several groups of 64 in flight (aligned dword loads from L2/HBM + byte
//     funnel); the others are resolved in stream order, 64 at a time, gated by a bitmap of
//     pending destination bytes; long / self-overlapping copies use the whole wavefront.
//   * the tile is flushed to HBM with 16-byte-per-lane coalesced stores.  HBM traffic is the
//     algorithmic C + D bytes plus the history reads that miss L2.

#ifndef DEBIG_T
#define DEBIG_T 4096 /* output tile bytes (multiple of 2048) */
#endif
#define DEBIG_TSLACK 272 /* >= 258 + 3, multiple of 16 */
#ifndef SEG_BYTES
#define SEG_BYTES 68 /* 17 dwords: odd dword stride spreads lanes over LDS banks */
#endif
#define SEG_BITS (SEG_BYTES * 8)
#define WIN_BYTES (64 * SEG_BYTES)
#define STAGE_BYTES (WIN_BYTES + 48)
#define STAGE_CHUNKS (STAGE_BYTES / 16)
// Segment size by workgroup width.  A window ends at end-of-block, so it should not be much
// larger than a typical block (16384 tokens, about 11 KB of image data): from 8 wavefronts up
// the segments are halved instead of the window doubled, which also halves every lane's serial
// scan -- what a lone, latency-bound stream needs.
template <int NW> struct SegCfg {
    static constexpr uint32_t BYTES = NW >= 8 ? SEG_BYTES / 2 : SEG_BYTES;
    static constexpr uint32_t BITS = 8u * BYTES;
    static constexpr uint32_t WIN = 64u * NW * BYTES; /* bytes of input one window covers */
    // Half-size segments are too short for a guessed start to fall into step with the real
    // symbol sequence (6.1 rounds per window instead of 3.6 on image data), so the first,
    // positions-only round starts one segment EARLIER and runs through the lane's own segment:
    // lanes arrive synchronised, the later rounds stay short.
    static constexpr uint32_t LEAD_BITS = NW >= 8 ? BITS : 0u;
};
// Width of the literal/length direct table, by workgroup width.  Real encoders' tables have
// many codes of 10..12 bits (the reference's sample PNGs: config 3 inflate 61.7 ms with 9 bits,
// 55.1 with 10, 49.8 with 11), but the table costs LDS: with one wavefront per workgroup 10
// bits keep 8 workgroups per CU (19.2 KB each) while 11 drop it to 6 and the headline by a
// third; the multi-wavefront workgroups have LDS to spare.
#ifndef PB_LIT_1
#define PB_LIT_1 10
#endif
#ifndef PB_LIT_MW
#define PB_LIT_MW 11
#endif
template <int NW> struct TabCfg {
    static constexpr uint32_t PBL = NW >= 2 ? PB_LIT_MW : PB_LIT_1;
};
// Distance direct table: 9 bits.  Measured (4096 x 64 KiB): dynamic-Huffman text 125.5 -> 132.4
// GB/s, image rows 77.7 -> 79.9, the config-5 gzip shard 149.3 -> 157.9, fixed-Huffman 148.4 ->
// 146.3 (its 5-bit distance codes gain nothing); 10 bits costs occupancy (dynamic 99.7).
#ifndef PB_DIST
#define PB_DIST 9
#endif
#define MPOS_CAP 704 /* >= 2048 / 3 match starts per 2048-byte span */

enum { FL_CONT = 0, FL_EOB = 1, FL_TAIL = 2, FL_ERR = 3 };
enum { CODE_LIT = 0, CODE_DIST = 1, CODE_CL = 2 };

#define SORT_BASE(c) ((c) == CODE_LIT ? 0u : (c) == CODE_DIST ? 288u : 320u)
// decode tables of the current block (one copy per wavefront, in LDS)
template <uint32_t PBL, class ENT = uint32_t, uint32_t SUBN_ = 256> struct __attribute__((aligned(16))) CodeTabsT {
    static constexpr uint32_t SUBN = SUBN_;
    ENT lit_tab[1u << PBL];     /* see mk_lit_entry  (Fmt32) / Fmt16::lit  */
    ENT dist_tab[1 << PB_DIST]; /* see mk_dist_entry (Fmt32) / Fmt16::dist */
    /* second-level tables of the codes longer than the direct tables: a direct-table slot whose
     * index is the first PBL (PB_DIST) bits of such codes holds a LINK {base, k}; the symbol is
     * sub_tab[base + next k bits].  Real encoders' tables have many 11..15-bit codes (about 1 % of
     * the symbols of a photo PNG): with 64..512 lanes in step nearly every loop iteration has a
     * lane on one, so the long-code path must be one more look-up, not a search. */
    ENT sub_tab[SUBN_];
    uint32_t sub_used;
    uint16_t sorted[288 + 32 + 20];  /* symbols sorted by (length, symbol): litlen | dist | cl */
    uint16_t first[3][16];           /* canonical first code of each length */
    uint16_t count[3][16];
    uint16_t offs[3][16];
    uint32_t qmin[3], qmax[3];
    /* index masks of lit_tab / dist_tab for the current block: min(table bits, longest code
     * present) bits.  A code with at most m bits fills the table periodically, so its first 2^m
     * entries are a complete table: a fixed-Huffman block indexes 512 literal and 32 distance
     * entries (the latter free of LDS bank conflicts) whatever the table size is. */
    uint32_t mask[2];
};

// LDS of one workgroup of NW wavefronts working on ONE stream (NW = 1: the default kernel;
// NW = 4: debig_inflate_mw_kernel for few-large-stream batches).  The window, the output tile
// and their bitmaps scale with NW; the decode tables are shared.
struct Fmt32; /* table entry format of these kernels, below */
template <int NW_> struct __attribute__((aligned(16))) WaveLdsT {
    static constexpr int NW = NW_;
    static constexpr uint32_t WIN_B = SegCfg<NW_>::WIN; /* bytes of input one staged window covers */
    typedef Fmt32 Fmt;
    uint8_t tile[DEBIG_T * NW + DEBIG_TSLACK];
    uint32_t inwin[(SegCfg<NW>::WIN + 48) / 4];
    uint32_t bitmap[DEBIG_T * NW / 32 + 16]; /* match starts left by pass 2 (source at least partly in the tile) */
    uint32_t farmap[DEBIG_T * NW / 32 + 16]; /* match starts whose whole source is already flushed to HBM */
    uint32_t pend[(DEBIG_T * NW + DEBIG_TSLACK) / 32 + 2]; /* bytes of not yet copied matches */
    CodeTabsT<TabCfg<NW>::PBL, uint32_t, (NW_ >= 2 ? 1024u : 256u)> t;
    uint16_t mpos[NW][MPOS_CAP]; /* per wavefront: match positions of the span being processed */
    uint8_t lens[320 + 144]; /* code lengths of the current dynamic header (+ run overshoot) */
    uint32_t cl_tab[1 << 7]; /* code-length code: direct table {len | sym << 16} */
    uint32_t cl_len[19];
    uint32_t cl_code[19];
    uint32_t cl_used[19];
    uint32_t internal_err; /* resolve_matches: a wavefront gave up polling (DEBIG_E_INTERNAL) */
};
typedef WaveLdsT<1> WaveLds;

#ifdef DEBIG_EMU
static unsigned long long debig_emu_slow_probes; /* emulator only: lengths tried by huff_slow's canonical probe (tests/test_emu_table_shapes.py) */
#define DEV_INLINE static inline
#define DEV_MEMBER static inline
#define DEV_MEMBER_INLINE inline
#define DEV_NOINLINE static
#define DEV_UNROLL
static inline uint8_t ld_hist_u8(const uint8_t *p) { return *p; }
static inline void wave_mem_fence() {}
static inline uint32_t ld_hist_u32(const uint32_t *p) { return *p; }
static inline uint32_t alignbyte32(uint32_t hi, uint32_t lo, uint32_t nbytes)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (nbytes & 3u)));
}
static inline uint4 ld_global_u4(const uint8_t *p)
{
    uint4 v;
    memcpy(&v, p, 16);
    return v;
}
static inline void st_global_u4(uint8_t *p, uint4 v) { memcpy(p, &v, 16); }
#else
#define DEV_INLINE __device__ __forceinline__
#define DEV_MEMBER static __device__ __forceinline__
#define DEV_MEMBER_INLINE __device__ __forceinline__
#define DEV_NOINLINE __device__ __attribute__((noinline))
#define DEV_UNROLL _Pragma("unroll")
// history bytes were written by this wavefront earlier: read them from L2, never from a
// possibly stale L1 line (MI355X_MICROARCH.md: sc1 loads bypass L1)
DEV_INLINE uint8_t ld_hist_u8(const uint8_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV_INLINE void wave_mem_fence() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
DEV_INLINE uint32_t ld_hist_u32(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV_INLINE uint32_t alignbyte32(uint32_t hi, uint32_t lo, uint32_t nbytes)
{
    return __builtin_amdgcn_alignbyte(hi, lo, nbytes);
}
DEV_INLINE uint4 ld_global_u4(const uint8_t *p) { return *reinterpret_cast<const uint4 *>(p); }
DEV_INLINE void st_global_u4(uint8_t *p, uint4 v) { *reinterpret_cast<uint4 *>(p) = v; }
#endif

DEV_INLINE uint32_t lane_id() { return threadIdx.x & 63u; }
DEV_INLINE uint32_t wave_id() { return threadIdx.x >> 6; }

// ordering of LDS traffic among the lanes of ONE wavefront.  With one wavefront per
// workgroup that is what __syncthreads() already is; in a multi-wavefront workgroup the
// other wavefronts must not be waited for (they may be in different code).
// the lanes of the CALLING wavefront only: LDS traffic before it is complete and visible behind it.  For a
// workgroup of one wavefront that is all __syncthreads() ever was; and a workgroup whose wavefronts run DIFFERENT
// code side by side (debig_strand_pipe_kernel: one scans, one replays) can only use this one.
DEV_INLINE void wave_local_sync()
{
#ifdef DEBIG_EMU
    __wave_barrier();
#else
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}
template <int NW> DEV_INLINE void wave_sync() { wave_local_sync(); }
// all wavefronts that work on the stream together: the workgroup when NW > 1, the calling wavefront when NW == 1
template <int NW> DEV_INLINE void group_sync()
{
    if (NW == 1) wave_local_sync();
    else __syncthreads();
}
// thread index among the 64 NW threads that work on the stream together
template <int NW> DEV_INLINE uint32_t group_tid() { return threadIdx.x & (64u * (uint32_t)NW - 1u); }

// Release / acquire of LDS data handed from one wavefront of the workgroup to another through
// the pending-byte bitmap (resolve_matches): copied tile bytes must be visible before their
// pending bits drop, and a reader that saw the bits clear must read the bytes after that.  (Measured,
// profiles/r04_mw_light_sync.txt: ordering them by the compiler alone, without the waits, has no effect
// on any workload -- the waits are implied by the rounds' data dependencies anyway.)
DEV_INLINE void lds_release_workgroup()
{
#ifndef DEBIG_EMU
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#endif
}
DEV_INLINE void lds_acquire_workgroup()
{
#ifndef DEBIG_EMU
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

// per-phase cycle accounting (diagnostic builds only: -DDEBIG_PROFILE)
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
#define PROF_DECL uint64_t prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; uint64_t prof_t0 = 0, prof_start = __builtin_amdgcn_s_memtime();
#define PROF_BEGIN() prof_t0 = __builtin_amdgcn_s_memtime()
#define PROF_END(i) prof_acc[i] += __builtin_amdgcn_s_memtime() - prof_t0
#define PROF_STORE(r) do { prof_acc[6] = __builtin_amdgcn_s_memtime() - prof_start; for (int pi = 0; pi < 8; pi++) (r).prof[pi] = (uint32_t)(prof_acc[pi] >> 4); } while (0)
#else
#define PROF_DECL
#define PROF_BEGIN()
#define PROF_END(i)
#define PROF_STORE(r) do { for (int pi = 0; pi < 8; pi++) (r).prof[pi] = 0; } while (0)
#endif

// value of lane `src` (the same in every lane: a v_readlane, no LDS round trip)
#ifdef DEBIG_EMU
#define wave_bcast_u32(v, src) ((uint32_t)__shfl((uint32_t)(v), (int)(src)))
#else
DEV_INLINE uint32_t wave_bcast_u32(uint32_t v, uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)src));
}
#endif

// exclusive prefix sum over the 64 lanes + the total
DEV_INLINE uint32_t wave_excl_scan_u32(uint32_t v, uint32_t *total)
{
#ifdef DEBIG_EMU
    uint32_t lane = lane_id();
    uint32_t x = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    *total = __shfl(x, 63);
    return x - v;
#else
    // DPP: shifts inside the rows of 16, then the row broadcasts (no LDS permutes: 12 VALU
    // instructions instead of six ds_bpermute round trips)
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111 /* row_shr:1 */, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112 /* row_shr:2 */, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114 /* row_shr:4 */, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118 /* row_shr:8 */, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142 /* row_bcast:15 */, 0xA, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143 /* row_bcast:31 */, 0xC, 0xF, false);
    *total = (uint32_t)__builtin_amdgcn_readlane(x, 63);
    return (uint32_t)x - v;
#endif
}

// ------------------------------------------------------------------ per-lane bit reader (LDS)
struct BitRd {
    uint64_t buf;
    uint32_t cnt;
    uint32_t nextw;
    int64_t pos; /* absolute bit position of the next unconsumed bit */
};

template <class LDS> DEV_INLINE void br_init(BitRd &b, const LDS &S, int64_t pos, int64_t org_bits)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    uint32_t local = (uint32_t)(pos - org_bits);
    b.nextw = local >> 5;
    uint32_t sh = local & 31u;
    b.buf = (uint64_t)(S.inwin[b.nextw++] >> sh);
    b.cnt = 32u - sh;
    b.pos = pos;
}
template <class LDS> DEV_INLINE void br_ensure(BitRd &b, const LDS &S)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    if (b.cnt <= 32u) {
        b.buf |= (uint64_t)S.inwin[b.nextw++] << b.cnt;
        b.cnt += 32u;
    }
}
DEV_INLINE uint32_t br_take(BitRd &b, uint32_t n)
{
    uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
    b.buf >>= n;
    b.cnt -= n;
    b.pos += n;
    return v;
}

// Table entries (u32), shared by the direct tables and the long-code fallback:
//   litlen: [3:0] code length (0 = no code) | [7:4] extra-bit count | [9:8] kind
//           (0 literal, 1 length, 2 end-of-block, 3 symbols 286/287) | [31:16] literal / base
//   dist  : [3:0] code length | [7:4] extra-bit count | [8] symbol > 29 | [31:16] base
// RFC 1951 3.2.5 base/extra values computed arithmetically (reference tables:
// src/inflate.c:716-779).
DEV_INLINE uint32_t mk_lit_entry(uint32_t sym, uint32_t l)
{
    if (sym < 256u) return l | (sym << 16);
    if (sym == 256u) return l | (2u << 8);
    if (sym > 285u) return l | (3u << 8);
    uint32_t lc = sym - 257u, ex, base;
    if (lc < 8u) { ex = 0; base = 3u + lc; }
    else if (lc == 28u) { ex = 0; base = 258u; }
    else { ex = (lc >> 2) - 1u; base = ((4u + (lc & 3u)) << ex) + 3u; }
    return l | (ex << 4) | (1u << 8) | (base << 16);
}
DEV_INLINE uint32_t mk_dist_entry(uint32_t sym, uint32_t l)
{
    if (sym > 29u) return l | (1u << 8);
    uint32_t ex, base;
    if (sym < 4u) { ex = 0; base = sym + 1u; }
    else { ex = (sym >> 1) - 1u; base = ((2u + (sym & 1u)) << ex) + 1u; }
    return l | (ex << 4) | (base << 16);
}
// Entry format as a type, so that the table builder and the long-code fallback serve kernels with
// a different (16-bit) format too (inflate_split_kernel.inc: Fmt16).
struct Fmt32 {
    typedef uint32_t T;
    static constexpr uint32_t CL_SHIFT = 16;
    DEV_MEMBER uint32_t lit(uint32_t sym, uint32_t l) { return mk_lit_entry(sym, l); }
    DEV_MEMBER uint32_t dist(uint32_t sym, uint32_t l) { return mk_dist_entry(sym, l); }
    DEV_MEMBER uint32_t cl(uint32_t sym, uint32_t l) { return l | (sym << 16); }
    /* entries with a zero length field: 0 = no code; LINK to a second-level table; SLOW = canonical probe */
    static constexpr uint32_t MAX_LINK_K = 6;
    DEV_MEMBER uint32_t link(uint32_t base, uint32_t k) { return 0xF000u | (k << 4) | (base << 16); }
    DEV_MEMBER uint32_t slowmark() { return 0xE000u; }
    DEV_MEMBER int is_link(uint32_t e) { return (e & 0xF00Fu) == 0xF000u; }
    DEV_MEMBER uint32_t link_k(uint32_t e) { return (e >> 4) & 15u; }
    DEV_MEMBER uint32_t link_base(uint32_t e) { return e >> 16; }
};
#define ENT_LEN(e) ((e) & 15u)
#define ENT_EXTRA(e) (((e) >> 4) & 15u)
#define ENT_KIND(e) (((e) >> 8) & 3u)
#define ENT_VAL(e) ((e) >> 16)

// long codes (or nothing): canonical probe, shortest length first like the reference's
// min..max loop (src/inflate.c:437-463).  Returns an entry, 0 when no code matches.
template <class LDS> DEV_INLINE uint32_t huff_slow(uint32_t bits, const LDS &S, int c, uint32_t e)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    typedef typename LDS::Fmt F;
    uint32_t pb = (c == CODE_LIT) ? TabCfg<NW>::PBL : PB_DIST;
    if (F::is_link(e)) /* the usual long code: one more look-up (0 = no code with these bits) */
        return S.t.sub_tab[F::link_base(e) + ((bits >> pb) & ((1u << F::link_k(e)) - 1u))];
    if (e == 0) return 0; /* no code starts with these bits */
    // SLOW mark (the second-level tables of a pathological code did not fit): canonical probe,
    // shortest length first like the reference's min..max loop (src/inflate.c:437-463)
    uint32_t lo = S.t.qmin[c] > pb + 1 ? S.t.qmin[c] : pb + 1;
    uint32_t hi = S.t.qmax[c] < 15u ? S.t.qmax[c] : 15u;
    uint32_t rv = __brev(bits);
    for (uint32_t len = lo; len <= hi; len++) {
#ifdef DEBIG_EMU
        debig_emu_slow_probes++;
#endif
        uint32_t code = rv >> (32u - len);
        uint32_t d = code - S.t.first[c][len];
        if (code >= S.t.first[c][len] && d < S.t.count[c][len]) {
            uint32_t sym = S.t.sorted[SORT_BASE(c) + S.t.offs[c][len] + d];
            return (c == CODE_LIT) ? F::lit(sym, len) : F::dist(sym, len);
        }
    }
    return 0;
}

// look one symbol up (the reader must hold >= 32 valid bits); 0 = no code (reference good=0)
template <class LDS> DEV_INLINE uint32_t huff_lookup(const BitRd &b, const LDS &S, int c)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    uint32_t bits = (uint32_t)b.buf;
    uint32_t e = (c == CODE_LIT) ? S.t.lit_tab[bits & S.t.mask[CODE_LIT]]
                                 : S.t.dist_tab[bits & S.t.mask[CODE_DIST]];
    if (ENT_LEN(e) == 0) e = huff_slow(bits, S, c, e);
    return e;
}

// code-length-code symbol (19 symbols, <= 7 bits) from its direct table; -1 = no code
template <class LDS> DEV_INLINE int cl_decode(BitRd &b, const LDS &S)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    uint32_t e = S.cl_tab[(uint32_t)b.buf & 127u];
    if ((e & 15u) == 0) return -1;
    br_take(b, e & 15u);
    return (int)(e >> LDS::Fmt::CL_SHIFT);
}

DEV_INLINE uint32_t funnel32(uint32_t hi, uint32_t lo, uint32_t sh)
{
#ifdef DEBIG_EMU
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u));
#else
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#endif
}

// The code lengths of the two alphabets (src/inflate.c:1416-1520: one code-length symbol at a
// time, 16 repeats the previous length, 17 / 18 are runs of zeros) decoded 64 BIT POSITIONS at a
// time: lane o looks up the symbol that would start at bit pos + o (one table look-up per lane
// instead of one per symbol for the whole wavefront), the chain of real symbol starts is then
// followed through the lanes with scalar reads (readlane), and the marked lanes place their
// lengths by a prefix sum over the repeat counts.  A 64 KiB dynamic stream spent 11 % of its scan
// in the serial loop this replaces (316 dependent look-ups of ~300 cycles each).
// Wave-uniform; every wavefront of a workgroup may run it (they write the same bytes).  hb is
// left behind the last symbol that was needed.  Returns 0, or 1 when a needed symbol has no code
// (the reference's good = 0).
template <class LDS> DEV_INLINE int decode_code_lengths(LDS &S, BitRd &hb, int64_t org_bits, uint32_t total)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    uint32_t pos = (uint32_t)(hb.pos - org_bits); /* window relative */
    uint32_t i = 0, prev = 0;
    int bad = 0;
    while (i < total) {
        const uint32_t lp = pos + lane, w = lp >> 5;
        const uint32_t bits = funnel32(S.inwin[w + 1], S.inwin[w], lp & 31u);
        const uint32_t e = S.cl_tab[bits & 127u];
        const uint32_t cl = e & 15u, sym = (uint32_t)(e >> LDS::Fmt::CL_SHIFT);
        const uint32_t nex = sym < 16u ? 0u : sym == 16u ? 2u : sym == 17u ? 3u : 7u;
        const uint32_t ex = (bits >> cl) & ((1u << nex) - 1u);
        const uint32_t rep_sym = sym < 16u ? 1u : sym == 18u ? 11u + ex : 3u + ex;
        const uint32_t adv = cl ? cl + nex : 0u; /* 0: no code starts with these bits */
        // the symbols that really start in [pos, pos + 64): a scalar walk over the lanes
        unsigned long long mark = 0;
        for (uint32_t o = 0; o < 64u;) {
            mark |= 1ull << o;
            const uint32_t a = wave_bcast_u32(adv, o);
            if (a == 0) break;
            o += a;
        }
        const int marked = (int)((mark >> lane) & 1ull);
        const uint32_t rep = (marked && cl) ? rep_sym : 0u;
        uint32_t tot;
        const uint32_t istart = i + wave_excl_scan_u32(rep, &tot);
        const int kept = marked && istart < total; /* the serial loop stops at i >= total */
        if (__any(kept && cl == 0)) { bad = 1; break; }
        // a 16 repeats the length in front of it: the nearest earlier symbol that is not a 16
        const unsigned long long keptm = __ballot(kept);
        const unsigned long long basem = __ballot(kept && sym != 16u) & lt_mask;
        uint32_t val = sym < 16u ? sym : 0u;
        {
            const uint32_t src = basem ? 63u - (uint32_t)__clzll((long long)basem) : 0u;
            const uint32_t pv = (uint32_t)__shfl((int)val, (int)src);
            if (sym == 16u) val = basem ? pv : prev;
        }
        if (kept && sym < 16u) S.lens[istart] = (uint8_t)val;
        unsigned long long rm = __ballot(kept && sym >= 16u);
        while (rm) { /* runs: one at a time, the lanes share the bytes */
            const uint32_t sl = (uint32_t)__ffsll((long long)rm) - 1u;
            rm &= rm - 1ull;
            const uint32_t ri = wave_bcast_u32(istart, sl), rn = wave_bcast_u32(rep, sl), rv = wave_bcast_u32(val, sl);
            for (uint32_t k = lane; k < rn; k += 64u) S.lens[ri + k] = (uint8_t)rv;
        }
        const uint32_t lk = 63u - (uint32_t)__clzll((long long)keptm); /* lane 0 is always kept */
        prev = wave_bcast_u32(val, lk);
        i = wave_bcast_u32(istart + rep, lk);
        pos += lk + wave_bcast_u32(adv, lk);
    }
    if (!bad) br_init(hb, S, org_bits + (int64_t)pos, org_bits);
    return bad;
}


// The HCLEN code lengths of the code-length code (3 bits each, in K_CL_ORDER: src/inflate.c:1262-1310),
// one per lane.  S.lens[0..18] must be zero; hb is left behind them.  Every wavefront may run it.
template <class LDS> DEV_INLINE void read_cl_lens(LDS &S, BitRd &hb, int64_t org_bits, uint32_t hclen)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = lane_id();
    const uint32_t pos = (uint32_t)(hb.pos - org_bits);
    if (lane < hclen) {
        const uint32_t lp = pos + 3u * lane, w = lp >> 5;
        const uint32_t bits = funnel32(S.inwin[w + 1], S.inwin[w], lp & 31u);
        // K_CL_ORDER, 5 bits per entry
        const uint32_t sym = lane < 12u ? (uint32_t)(0x22caa324e804a30ull >> (5u * lane)) & 31u
                                        : (uint32_t)(0x3c2e1346cull >> (5u * (lane - 12u))) & 31u;
        S.lens[sym] = (uint8_t)(bits & 7u);
    }
    br_init(hb, S, org_bits + (int64_t)(pos + 3u * hclen), org_bits);
}

// ------------------------------------------------------------------ table construction
#define PB_CL 7 /* code-length codes are at most 7 bits: one direct table, no fallback */

// inclusive prefix minimum / maximum over the lanes and the wave-wide reductions: DPP row shifts
// and row broadcasts (lanes that have no source keep the operation's identity), no LDS permutes
#ifdef DEBIG_EMU
DEV_INLINE uint32_t wave_incl_min_u32(uint32_t v)
{
    uint32_t lane = lane_id();
    for (uint32_t d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(v, d);
        if (lane >= d) v = o < v ? o : v;
    }
    return v;
}
DEV_INLINE uint32_t wave_incl_max_u32(uint32_t v)
{
    uint32_t lane = lane_id();
    for (uint32_t d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(v, d);
        if (lane >= d) v = o > v ? o : v;
    }
    return v;
}
DEV_INLINE uint32_t wave_min_u32(uint32_t v) { return __shfl(wave_incl_min_u32(v), 63); }
DEV_INLINE uint32_t wave_max_u32(uint32_t v) { return __shfl(wave_incl_max_u32(v), 63); }
#else
#define DEBIG_DPP_STEP(OP, IDENT, CTRL, ROWMASK)                                                          \
    {                                                                                                     \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)(IDENT), (int)v, CTRL, ROWMASK, 0xF, false); \
        v = OP;                                                                                           \
    }
DEV_INLINE uint32_t wave_incl_min_u32(uint32_t v)
{
    DEBIG_DPP_STEP(o < v ? o : v, 0xffffffffu, 0x111, 0xF)
    DEBIG_DPP_STEP(o < v ? o : v, 0xffffffffu, 0x112, 0xF)
    DEBIG_DPP_STEP(o < v ? o : v, 0xffffffffu, 0x114, 0xF)
    DEBIG_DPP_STEP(o < v ? o : v, 0xffffffffu, 0x118, 0xF)
    DEBIG_DPP_STEP(o < v ? o : v, 0xffffffffu, 0x142, 0xA)
    DEBIG_DPP_STEP(o < v ? o : v, 0xffffffffu, 0x143, 0xC)
    return v;
}
DEV_INLINE uint32_t wave_incl_max_u32(uint32_t v)
{
    DEBIG_DPP_STEP(o > v ? o : v, 0u, 0x111, 0xF)
    DEBIG_DPP_STEP(o > v ? o : v, 0u, 0x112, 0xF)
    DEBIG_DPP_STEP(o > v ? o : v, 0u, 0x114, 0xF)
    DEBIG_DPP_STEP(o > v ? o : v, 0u, 0x118, 0xF)
    DEBIG_DPP_STEP(o > v ? o : v, 0u, 0x142, 0xA)
    DEBIG_DPP_STEP(o > v ? o : v, 0u, 0x143, 0xC)
    return v;
}
DEV_INLINE uint32_t wave_min_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_min_u32(v), 63); }
DEV_INLINE uint32_t wave_max_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max_u32(v), 63); }
#endif

// Restates unpack_huffman (src/inflate.c:565-706) + huffman_to_hashmap (:494-557):
//   * a length >= n fails the stream (Q6)
//   * strict (streams with DEBIG_STREAM_NO_REF_GATES only): an over-subscribed set of lengths (Kraft sum above 1) fails the
//     stream as well.  The reference only asserts there, and without this every kernel would resolve the overlapping codes
//     by its own table layout: the same stream would end differently at different widths.  Wave-uniform like Q6.
//   * canonical codes for every non-zero length
//   * probe range [qmin,qmax] from the reference's if / else-if update in symbol order (Q7):
//     qmin = smallest non-zero length; qmax = the largest length among the symbols that are
//     NOT a strict new minimum when met in symbol order (and at least 1)
// Whole-wavefront construction: symbol i = 64 k + lane; per-length counts and the rank of each
// symbol inside its length class come from ballots, offsets from a 15-step prefix sum, the
// direct table is filled in parallel.  `lens` points into LDS, n <= 320.
// Returns 0 on the Q6 failure (wave-uniform).
template <class LDS> DEV_INLINE int build_code(LDS &S, int c, const uint8_t *lens, uint32_t n, const int strict = 0)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = lane_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    uint32_t len_k[5], rank_k[5];
    uint32_t run[16];
DEV_UNROLL
    for (int L = 0; L < 16; L++) run[L] = 0;
    int bad = 0;
    uint32_t running_min = 9999u, qmax = 1u;
    wave_sync<NW>();
DEV_UNROLL
    for (int k = 0; k < 5; k++) {
        uint32_t i = 64u * (uint32_t)k + lane;
        uint32_t l = i < n ? (uint32_t)lens[i] : 0u;
        bad |= (i < n) && (l >= n);
        l &= 15u;
        len_k[k] = l;
        rank_k[k] = 0;
DEV_UNROLL
        for (int L = 1; L < 16; L++) {
            unsigned long long bm = __ballot(l == (uint32_t)L);
            if (l == (uint32_t)L) rank_k[k] = run[L] + (uint32_t)__popcll(bm & lt_mask);
            run[L] += (uint32_t)__popcll(bm);
        }
        // Q7 bookkeeping: exclusive prefix minimum of the non-zero lengths, in symbol order
        uint32_t v = l ? l : 9999u;
        const uint32_t inc = wave_incl_min_u32(v);
        uint32_t excl = __shfl_up(inc, 1);
        if (lane == 0) excl = 9999u;
        uint32_t pm = excl < running_min ? excl : running_min;
        uint32_t cand = (l != 0 && l >= pm) ? l : 0u;
        uint32_t cm = wave_max_u32(cand);
        qmax = cm > qmax ? cm : qmax;
        uint32_t wm = wave_min_u32(v);
        running_min = wm < running_min ? wm : running_min;
    }
    if (__any(bad)) return 0;
    if (strict) { /* DEBIG_STREAM_NO_REF_GATES (plain RFC 1951): an over-subscribed set fails the stream, at every width alike */
        uint32_t kraft = 0;
DEV_UNROLL
        for (int L = 1; L < 16; L++) kraft += run[L] << (15 - L);
        if (kraft > (1u << 15)) return 0;
    }
    // canonical first codes / offsets (uniform: every lane computes the same 15 steps)
    {
        uint32_t code = 0, off = 0, prev = 0;
DEV_UNROLL
        for (int L = 1; L < 16; L++) {
            code = (code + prev) << 1;
            if (lane == 0) {
                S.t.first[c][L] = (uint16_t)code;
                S.t.count[c][L] = (uint16_t)run[L];
                S.t.offs[c][L] = (uint16_t)off;
            }
            off += run[L];
            prev = run[L];
        }
        if (lane == 0) {
            S.t.first[c][0] = 0;
            S.t.count[c][0] = 0;
            S.t.offs[c][0] = 0;
            S.t.qmin[c] = running_min;
            S.t.qmax[c] = qmax;
            if (c != CODE_CL) {
                uint32_t maxl = 1; /* longest code present, whether or not the probe range covers it */
DEV_UNROLL
                for (int L = 1; L < 16; L++) maxl = run[L] ? (uint32_t)L : maxl;
                const uint32_t tb = (c == CODE_LIT) ? TabCfg<NW>::PBL : (uint32_t)PB_DIST;
                S.t.mask[c] = (1u << (maxl < tb ? maxl : tb)) - 1u;
            }
        }
    }
    typedef typename LDS::Fmt F;
    typename F::T *tab = (c == CODE_LIT) ? S.t.lit_tab : (c == CODE_DIST) ? S.t.dist_tab : S.cl_tab;
    const uint32_t pb = (c == CODE_LIT) ? TabCfg<NW>::PBL : (c == CODE_DIST) ? PB_DIST : PB_CL;
    for (uint32_t k = lane; k < (1u << pb); k += 64) tab[k] = 0;
    wave_sync<NW>();
    const uint32_t qmin = running_min;
DEV_UNROLL
    for (int k = 0; k < 5; k++) {
        uint32_t l = len_k[k];
        if (l == 0) continue;
        uint32_t sym = 64u * (uint32_t)k + lane;
        uint32_t idx = (uint32_t)S.t.offs[c][l] + rank_k[k];
        S.t.sorted[SORT_BASE(c) + idx] = (uint16_t)sym;
        if (l > pb || l < qmin || l > qmax) continue;
        uint32_t code = (uint32_t)S.t.first[c][l] + rank_k[k];
        uint32_t r = __brev(code) >> (32u - l);
        uint32_t e = (c == CODE_LIT) ? F::lit(sym, l) : (c == CODE_DIST) ? F::dist(sym, l) : F::cl(sym, l);
        for (uint32_t q = r & ((1u << pb) - 1u); q < (1u << pb); q += (1u << l)) tab[q] = (typename F::T)e;
    }
    wave_sync<NW>();
    // ---- second-level tables for the codes longer than the direct table (see CodeTabsT::sub_tab).
    // In canonical (= sorted) order the codes that share their first pb bits are neighbours and
    // their lengths do not decrease, so the LAST code of such a run knows the run's table size.
    uint32_t total_codes = 0, maxl = 0;
DEV_UNROLL
    for (int L = 1; L < 16; L++) { total_codes += run[L]; maxl = run[L] ? (uint32_t)L : maxl; }
    if (c != CODE_CL && maxl > pb) { /* wave-uniform */
        constexpr uint32_t SUBN = decltype(S.t)::SUBN;
        typename F::T *sub = S.t.sub_tab;
        uint32_t running = (c == CODE_LIT) ? 0u : S.t.sub_used; /* the distance code allocates behind the literal/length code */
        for (uint32_t k5 = 0; 64u * k5 < total_codes; k5++) {
            const uint32_t pos = 64u * k5 + lane, pos2 = pos + 1u;
            const int in1 = pos < total_codes, in2 = pos2 < total_codes;
            const uint32_t sym1 = in1 ? (uint32_t)S.t.sorted[SORT_BASE(c) + pos] : 0u;
            const uint32_t sym2 = in2 ? (uint32_t)S.t.sorted[SORT_BASE(c) + pos2] : 0u;
            const uint32_t l1 = in1 ? ((uint32_t)lens[sym1] & 15u) : 0u, l2 = in2 ? ((uint32_t)lens[sym2] & 15u) : 0u;
            const int long1 = in1 && l1 > pb && l1 >= qmin && l1 <= qmax;
            const int long2 = in2 && l2 > pb && l2 >= qmin && l2 <= qmax;
            const uint32_t code1 = (uint32_t)S.t.first[c][l1] + (pos - (uint32_t)S.t.offs[c][l1]);
            const uint32_t code2 = (uint32_t)S.t.first[c][l2] + (pos2 - (uint32_t)S.t.offs[c][l2]);
            const uint32_t pre1 = long1 ? code1 >> (l1 - pb) : 0u;
            const uint32_t pre2 = long2 ? code2 >> (l2 - pb) : 0xffffffffu;
            const int last = long1 && pre2 != pre1;
            const uint32_t size = last ? 1u << (l1 - pb) : 0u;
            uint32_t tot;
            const uint32_t base = running + wave_excl_scan_u32(size, &tot);
            running += tot;
            if (last) {
                const uint32_t pidx = __brev(pre1) >> (32u - pb);
                if (base + size <= SUBN && l1 - pb <= F::MAX_LINK_K) {
                    tab[pidx] = (typename F::T)F::link(base, l1 - pb);
                    for (uint32_t q = 0; q < size; q++) sub[base + q] = 0;
                } else {
                    tab[pidx] = (typename F::T)F::slowmark();
                }
            }
        }
        if (lane == 0) S.t.sub_used = running < SUBN ? running : SUBN;
        wave_sync<NW>();
DEV_UNROLL
        for (int k = 0; k < 5; k++) {
            const uint32_t l = len_k[k];
            if (l <= pb || l < qmin || l > qmax) continue;
            const uint32_t sym = 64u * (uint32_t)k + lane;
            const uint32_t code = (uint32_t)S.t.first[c][l] + rank_k[k];
            const uint32_t r = __brev(code) >> (32u - l);
            const uint32_t e0 = tab[r & ((1u << pb) - 1u)];
            if (!F::is_link(e0)) continue;
            const uint32_t e = (c == CODE_LIT) ? F::lit(sym, l) : F::dist(sym, l);
            const uint32_t bs = F::link_base(e0), kk = F::link_k(e0);
            for (uint32_t q = r >> pb; q < (1u << kk); q += 1u << (l - pb)) sub[bs + q] = (typename F::T)e;
        }
        wave_sync<NW>();
    } else if (c == CODE_LIT && lane == 0) {
        S.t.sub_used = 0;
    }
    return 1;
}

// ------------------------------------------------------------------ input staging
// Stage STAGE_BYTES of the stream, starting at the 16-byte aligned global address at or
// below byte `from_byte`, into S.inwin.  Bytes outside [0, in_len) read as zero (the
// reference reads whatever follows the input: only corrupt streams can tell).  Returns the
// stream-relative byte index of inwin[0] (may be negative by up to 15).
template <class LDS> DEV_INLINE int64_t stage_window(LDS &S, const uint8_t *in, uint64_t in_len, int64_t from_byte)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = group_tid<NW>(); /* all NW wavefronts stage */
    uintptr_t ga = (uintptr_t)(in + from_byte);
    int64_t base = from_byte - (int64_t)(ga & 15u);
    group_sync<NW>();
    for (uint32_t c = lane; c < (LDS::WIN_B + 48) / 16; c += 64 * NW) {
        int64_t idx = base + 16 * (int64_t)c;
        uint4 v;
        if (idx >= 0 && (uint64_t)idx + 16 <= in_len) {
            v = ld_global_u4(in + idx);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int k = 0; k < 16; k++) {
                int64_t i = idx + k;
                if (i >= 0 && (uint64_t)i < in_len) w[k >> 2] |= (uint32_t)in[i] << (8 * (k & 3));
            }
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *reinterpret_cast<uint4 *>(&S.inwin[4 * c]) = v;
    }
    group_sync<NW>();
    return base;
}

// The staged window stays valid until the next stage_window(): a caller that only needs `need`
// bytes from `from_byte` (a block header, the probe of a short block) keeps using it, which
// matters for streams made of tiny blocks (encoders that flush every row): hundreds of blocks
// fit one window.  aligned = 1: the caller needs inwin[0] within 15 bytes below from_byte (the
// segment grid of pass 1 starts there).
template <class LDS> DEV_INLINE int64_t stage_window_cached(LDS &S, const uint8_t *in, uint64_t in_len,
                                                        int64_t from_byte, uint32_t need, int aligned,
                                                        int64_t &base, int &valid)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const int64_t span = (int64_t)LDS::WIN_B + 48;
    const int hit = valid && from_byte >= base && from_byte + (int64_t)need <= base + span &&
                    (!aligned || from_byte - base < 16);
    if (!hit) {
        base = stage_window(S, in, in_len, from_byte);
        valid = 1;
    }
    return base;
}
#define DEBIG_HEADER_NEED 352u /* block header: <= 17 + 19*3 + 320*7 bits, + bit reader look-ahead */
#define DEBIG_PROBE_NEED (SEG_BYTES + 24u)

// ------------------------------------------------------------------ output tile
struct OutState {
    uint8_t *out;      /* recipient */
    uint8_t *out2;     /* two-plane replay of the chunk path (inflate_chunk_kernel.inc) only: plane B */
    uint64_t out_cap;  /* recipient_size */
    int64_t tile_base; /* absolute output position of tile[0]; (out + tile_base) % 16 == 0 */
    int64_t lds_from;  /* positions >= lds_from live in the LDS tile, older ones in HBM */
    int64_t outpos;    /* bytes produced and fully resolved so far */
    /* debig_png_fused_kernel only: where the LZ77 wavefront tells the de-filter wavefronts of its workgroup how many
     * bytes of the recipient are final and in L2 (lz_publish), never more than pub_cap (the decode_png aliasing
     * replay rewrites what lies behind it) */
    volatile uint32_t *pub = nullptr;
    int64_t pub_cap = 0;
};

DEV_INLINE int64_t align_anchor(const uint8_t *out, int64_t pos)
{
    uintptr_t a = (uintptr_t)out + (uintptr_t)pos;
    return pos - (int64_t)(a & 15u);
}

// write tile bytes for absolute positions [from, to) to HBM (coalesced 16 B per lane body)
// fence = 0: the caller waits for the stores itself (wave_mem_fence) before anything reads them back
template <class LDS> DEV_INLINE void flush_range(LDS &S, OutState &O, int64_t from, int64_t to, int fence = 1)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = group_tid<NW>(); /* all NW wavefronts flush */
    group_sync<NW>();
    if (to > from) {
        uint8_t *g = O.out + from;
        uint32_t rel = (uint32_t)(from - O.tile_base);
        uint64_t n = (uint64_t)(to - from);
        uint32_t head = (uint32_t)((16u - ((uintptr_t)g & 15u)) & 15u);
        if (head > n) head = (uint32_t)n;
        if (lane < head) g[lane] = S.tile[rel + lane];
        uint64_t body = (n - head) & ~(uint64_t)15;
        for (uint64_t off = (uint64_t)lane * 16; off < body; off += 1024u * NW) {
            uint4 v = *reinterpret_cast<const uint4 *>(&S.tile[rel + head + off]);
            st_global_u4(g + head + off, v);
        }
        uint32_t tail = (uint32_t)(n - head - body);
        if (lane < tail) g[head + body + lane] = S.tile[rel + head + body + lane];
    }
    if (fence) wave_mem_fence();
    group_sync<NW>();
}

// flush everything produced so far and restart the tile at outpos
template <class LDS> DEV_INLINE void flush_all(LDS &S, OutState &O)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    flush_range(S, O, O.lds_from, O.outpos);
    O.lds_from = O.outpos;
    O.tile_base = align_anchor(O.out, O.outpos);
}

// one history byte at absolute position p (p < current write position)
template <class LDS> DEV_INLINE uint8_t hist_byte(const LDS &S, const OutState &O, int64_t p)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    if (p >= O.lds_from) return S.tile[p - O.tile_base];
    return ld_hist_u8(O.out + p);
}

// One match copied by all 64 lanes of a wavefront (the long, self-overlapping and flush-straddling
// matches of the resolve loops, one at a time): tile position lp, length ll (3..258), distance ld,
// all wavefront-uniform.  Real PNG files are full of these (runs: distance 1..4, length up to
// 258), so the per-byte work is kept small: the source index of a self-overlapping match is
// k mod ld by one multiplication (M = ceil(2^20 / ld), exact for k < 320), a source that lies
// wholly in the tile is read without the tile / HBM test per byte.
template <class LDS> DEV_INLINE void copy_match_wave(LDS &S, const OutState &O, uint32_t lp, uint32_t ll, uint32_t ld)
{
    const uint32_t lane = lane_id();
    const int64_t ls = O.tile_base + (int64_t)lp - (int64_t)ld; /* absolute position of the source */
    const int overlap = ld < ll;
    const uint32_t M = overlap ? ((1u << 20) + ld - 1u) / ld : 0u;
    const int in_tile = ls >= O.lds_from;
    const uint32_t sr = (uint32_t)(ls - O.tile_base); /* tile relative, when in_tile */
    uint8_t tmp[5];
    DEV_UNROLL
    for (uint32_t it = 0; it < 5; it++) {
        const uint32_t k = it * 64u + lane;
        if (k < ll) {
            const uint32_t kk = overlap ? k - ((k * M) >> 20) * ld : k;
            tmp[it] = in_tile ? S.tile[sr + kk] : hist_byte(S, O, ls + kk);
        }
    }
    DEV_UNROLL
    for (uint32_t it = 0; it < 5; it++) {
        const uint32_t k = it * 64u + lane;
        if (k < ll) S.tile[lp + k] = tmp[it];
    }
}

// ------------------------------------------------------------------ LZ77 resolve
// pending-byte bitmap helpers: bit i of S.pend <=> tile byte i is the destination of a match
// that has not been copied yet.  Ranges are tile relative and at most 258 long.
// masks of a range of <= 32 bits starting at bit p: word p>>5 gets m0, the next one m1
DEV_INLINE void range_masks(uint32_t p, uint32_t len, uint32_t &m0, uint32_t &m1)
{
    uint64_t m = ((len >= 32u ? 0xffffffffull : ((1ull << len) - 1ull))) << (p & 31u);
    m0 = (uint32_t)m;
    m1 = (uint32_t)(m >> 32);
}
template <class LDS> DEV_INLINE void pend_set(LDS &S, uint32_t p, uint32_t len)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    if (len <= 32u) {
        uint32_t m0, m1;
        range_masks(p, len, m0, m1);
        atomicOr(&S.pend[p >> 5], m0);
        if (m1) atomicOr(&S.pend[(p >> 5) + 1], m1);
        return;
    }
    uint32_t w = p >> 5, sh = p & 31u;
    while (len) {
        uint32_t n = 32u - sh < len ? 32u - sh : len;
        uint32_t m = (n == 32u ? ~0u : ((1u << n) - 1u)) << sh;
        atomicOr(&S.pend[w], m);
        len -= n;
        w++;
        sh = 0;
    }
}
template <class LDS> DEV_INLINE void pend_clear(LDS &S, uint32_t p, uint32_t len)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    if (len <= 32u) {
        uint32_t m0, m1;
        range_masks(p, len, m0, m1);
        atomicAnd(&S.pend[p >> 5], ~m0);
        if (m1) atomicAnd(&S.pend[(p >> 5) + 1], ~m1);
        return;
    }
    uint32_t w = p >> 5, sh = p & 31u;
    while (len) {
        uint32_t n = 32u - sh < len ? 32u - sh : len;
        uint32_t m = (n == 32u ? ~0u : ((1u << n) - 1u)) << sh;
        atomicAnd(&S.pend[w], ~m);
        len -= n;
        w++;
        sh = 0;
    }
}
template <class LDS> DEV_INLINE int pend_any(const LDS &S, uint32_t p, uint32_t len)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    if (len <= 32u) {
        uint32_t m0, m1;
        range_masks(p, len, m0, m1);
        return ((S.pend[p >> 5] & m0) | (S.pend[(p >> 5) + 1] & m1)) != 0;
    }
    uint32_t w = p >> 5, sh = p & 31u, acc = 0;
    while (len) {
        uint32_t n = 32u - sh < len ? 32u - sh : len;
        uint32_t m = (n == 32u ? ~0u : ((1u << n) - 1u)) << sh;
        acc |= S.pend[w] & m;
        len -= n;
        w++;
        sh = 0;
    }
    return acc != 0;
}

/* positions-only rounds of pass 1 before the full scan: a second one makes the full-cost
 * fix-up round rare.  Measured (4096 x 64 KiB): fixed-Huffman 136.9 -> 142.1 GB/s with 2, but
 * dynamic blocks 119.5 -> 117.2 and image data 72.5 -> 68.9, hence per block type. */
#ifndef DEBIG_POS_ROUNDS_FIXED
#define DEBIG_POS_ROUNDS_FIXED 2u
#endif
#ifndef DEBIG_POS_ROUNDS_DYNAMIC
#define DEBIG_POS_ROUNDS_DYNAMIC 1u
#endif
#define FAR_DEPTH 4
// Copy every match of tile-relative [from_rel, to_rel) whose source lies entirely in the
// already flushed output (S.farmap).  These have no ordering constraints at all -- their
// sources are final -- so FAR_DEPTH groups of 64 are kept in flight to cover the L2/HBM
// latency: aligned dword loads (L1 bypass), a byte funnel shift, byte stores into the tile.
template <class LDS> DEV_INLINE void far_copy(LDS &S, OutState &O, uint32_t from_rel, uint32_t to_rel)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = lane_id();
    for (uint32_t span = (from_rel >> 11) + wave_id(); span < ((to_rel + 2047u) >> 11); span += NW) {
        wave_sync<NW>();
        uint32_t wbase = span * 64u + lane;
        uint32_t w = S.farmap[wbase];
        uint32_t p0 = wbase * 32u;
        if (p0 + 32u <= from_rel || p0 >= to_rel) w = 0;
        else {
            if (p0 < from_rel) w &= ~0u << (from_rel - p0);
            if (p0 + 32u > to_rel) w &= (1u << (to_rel - p0)) - 1u;
        }
        S.farmap[wbase] = 0;
        uint32_t total;
        uint32_t pre = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        {
            uint32_t k = pre, ww = w;
            while (ww) {
                uint32_t bit = (uint32_t)__ffs(ww) - 1u;
                ww &= ww - 1u;
                S.mpos[wave_id()][k++] = (uint16_t)(p0 + bit);
            }
        }
        wave_sync<NW>();
        for (uint32_t g0 = 0; g0 < total; g0 += 64u * FAR_DEPTH) {
            uint32_t mp[FAR_DEPTH], mlen[FAR_DEPTH], msh[FAR_DEPTH];
            uint32_t t[FAR_DEPTH][5];
            int64_t msrc[FAR_DEPTH];
            DEV_UNROLL
            for (int d = 0; d < FAR_DEPTH; d++) {
                uint32_t q = g0 + (uint32_t)d * 64u + lane;
                mp[d] = 0; mlen[d] = 0; msh[d] = 0; msrc[d] = 0;
                if (q < total) {
                    uint32_t p = S.mpos[wave_id()][q];
                    uint32_t len = (uint32_t)S.tile[p] + 3u;
                    uint32_t dist = ((uint32_t)S.tile[p + 1] | ((uint32_t)S.tile[p + 2] << 8)) + 1u;
                    mp[d] = p; mlen[d] = len;
                    msrc[d] = O.tile_base + (int64_t)p - (int64_t)dist;
                    uintptr_t a = (uintptr_t)(O.out + msrc[d]);
                    msh[d] = (uint32_t)(a & 3u);
                    if (len <= 16u) {
                        const uint32_t *base = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
                        uint32_t ndw = (msh[d] + len + 3u) >> 2;
                        DEV_UNROLL
                        for (uint32_t i = 0; i < 5; i++)
                            if (i < ndw) t[d][i] = ld_hist_u32(base + i);
                    }
                }
            }
            DEV_UNROLL
            for (int d = 0; d < FAR_DEPTH; d++) {
                // byte stores in tiers of 4 / 4 / 8: most matches are 3..8 bytes long, so the
                // upper tiers are usually skipped by the whole wavefront
                const uint32_t len = mlen[d];
                const int mine = len != 0 && len <= 16u;
                uint32_t v[4] = {0, 0, 0, 0};
                if (mine) {
                    DEV_UNROLL
                    for (uint32_t i = 0; i < 4; i++) v[i] = alignbyte32(t[d][i + 1], t[d][i], msh[d]);
                    S.tile[mp[d]] = (uint8_t)v[0]; S.tile[mp[d] + 1] = (uint8_t)(v[0] >> 8);
                    S.tile[mp[d] + 2] = (uint8_t)(v[0] >> 16);
                    if (len > 3u) S.tile[mp[d] + 3] = (uint8_t)(v[0] >> 24);
                }
                if (__any(mine && len > 4u)) {
                    if (mine) {
                        DEV_UNROLL
                        for (uint32_t k = 4; k < 8; k++)
                            if (k < len) S.tile[mp[d] + k] = (uint8_t)(v[1] >> (8u * (k & 3u)));
                    }
                    if (__any(mine && len > 8u)) {
                        if (mine) {
                            DEV_UNROLL
                            for (uint32_t k = 8; k < 16; k++)
                                if (k < len) S.tile[mp[d] + k] = (uint8_t)(v[k >> 2] >> (8u * (k & 3u)));
                        }
                    }
                }
            }
            // long far matches: one at a time, all 64 lanes copy
            DEV_UNROLL
            for (int d = 0; d < FAR_DEPTH; d++) {
                unsigned long long lm = __ballot(mlen[d] > 16u);
                while (lm) {
                    int sl = __ffsll(lm) - 1;
                    lm &= lm - 1;
                    uint32_t lp = __shfl(mp[d], sl);
                    uint32_t ll = __shfl(mlen[d], sl);
                    int64_t ls = __shfl(msrc[d], sl);
                    uint8_t tmp[5];
                    DEV_UNROLL
                    for (uint32_t it = 0; it < 5; it++) {
                        uint32_t k = it * 64u + lane;
                        if (k < ll) tmp[it] = ld_hist_u8(O.out + ls + k);
                    }
                    DEV_UNROLL
                    for (uint32_t it = 0; it < 5; it++) {
                        uint32_t k = it * 64u + lane;
                        if (k < ll) S.tile[lp + k] = tmp[it];
                    }
                }
            }
        }
    }
    wave_sync<NW>();
}

// Copy of a short (3..16 bytes), non-overlapping match whose source lies in the LDS tile, by
// its own lane: 5 dword reads + byte funnel instead of up to 16 byte reads, and the byte stores
// in tiers (most matches are 3..8 bytes long, so the upper tiers are usually skipped by the
// whole wavefront).  `mine` selects the lanes that copy; must be called by the whole wavefront.
template <class LDS> DEV_INLINE void copy_short_match(LDS &S, int mine, uint32_t p, uint32_t len, uint32_t sr)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    if (!__any(mine)) return;
    uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (mine) {
        const uint32_t *tw = reinterpret_cast<const uint32_t *>(S.tile);
        const uint32_t q = sr >> 2, sh = sr & 3u;
        const uint32_t a0 = tw[q], a1 = tw[q + 1], a2 = tw[q + 2], a3 = tw[q + 3], a4 = tw[q + 4];
        v0 = alignbyte32(a1, a0, sh); v1 = alignbyte32(a2, a1, sh);
        v2 = alignbyte32(a3, a2, sh); v3 = alignbyte32(a4, a3, sh);
        S.tile[p] = (uint8_t)v0; S.tile[p + 1] = (uint8_t)(v0 >> 8); S.tile[p + 2] = (uint8_t)(v0 >> 16);
        if (len > 3u) S.tile[p + 3] = (uint8_t)(v0 >> 24);
    }
    if (!__any(mine && len > 4u)) return;
    if (mine) {
DEV_UNROLL
        for (uint32_t k = 4; k < 8; k++)
            if (k < len) S.tile[p + k] = (uint8_t)(v1 >> (8u * (k & 3u)));
    }
    if (!__any(mine && len > 8u)) return;
    if (mine) {
DEV_UNROLL
        for (uint32_t k = 8; k < 16; k++)
            if (k < len) S.tile[p + k] = (uint8_t)((k < 12 ? v2 : v3) >> (8u * (k & 3u)));
    }
}

// Resolve every match whose start lies in tile-relative [from_rel, to_rel).
// Matches were left by pass 2 as {len-3, (dist-1) lo, (dist-1) hi} in their first three
// destination bytes plus a bit in S.bitmap.  Replaces the reference's copy
// (src/inflate.c:1842-1897; byte-by-byte semantics, overlap replicates).
//
//   phase A  the destination bytes of every match in the range are marked pending (S.pend),
//            each wavefront for its own 2 KiB spans, straight from the bitmap words;
//   -------- workgroup barrier
//   phase B  every wavefront works through its spans with a SLIDING WINDOW of 64 matches, one
//            per lane: a match is copied as soon as none of its source bytes is pending --
//            whichever match or wavefront owns them -- and a lane that has finished takes the
//            span's next match in the same round.  Real data has dependency chains a few
//            matches deep (a photo PNG: about 5 within any 64 consecutive matches); with fixed
//            groups of 64 every group paid its whole chain depth in rounds while the
//            independent matches behind it waited; the window keeps the lanes occupied.
// The earliest unresolved match of a span is always in the window and never waits for
// anything later, so every round makes progress; across wavefronts the bitmap is polled (no
// barriers inside, bounded idle polls).  Sources older than the tile come from the flushed
// output (HBM/L2).  Must be called by all threads of the workgroup.
DEV_INLINE void resolve_poll_pause()
{
#ifndef DEBIG_EMU
    __builtin_amdgcn_s_sleep(2);
#endif
}
DEV_INLINE uint32_t span_word(uint32_t w, uint32_t p0, uint32_t from_rel, uint32_t to_rel)
{
    if (p0 + 32u <= from_rel || p0 >= to_rel) return 0;
    if (p0 < from_rel) w &= ~0u << (from_rel - p0);
    if (p0 + 32u > to_rel) w &= (1u << (to_rel - p0)) - 1u;
    return w;
}

#ifndef DEBIG_RESOLVE_IDLE_BOUND
#define DEBIG_RESOLVE_IDLE_BOUND (1u << 22)
#endif
// Returns 0, or 1 (the same value in every thread) when a wavefront exhausted its idle polls:
// the caller fails the stream with DEBIG_E_INTERNAL.  idle_bound: DEBIG_RESOLVE_IDLE_BOUND, or 0
// for streams flagged DEBIG_STREAM_FAULT_INJECT_IDLE (test hook: the first idle poll gives up).
template <class LDS> DEV_INLINE int resolve_matches(LDS &S, OutState &O, uint32_t from_rel, uint32_t to_rel,
                                                 uint32_t idle_bound = DEBIG_RESOLVE_IDLE_BOUND)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = lane_id();
    const uint32_t wv = wave_id();
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int64_t lds_rel0 = O.lds_from - O.tile_base; /* tile bytes below this are not in LDS */
    const uint32_t span0 = from_rel >> 11, span1 = (to_rel + 2047u) >> 11;
    // phase A
    for (uint32_t span = span0 + wv; span < span1; span += NW) {
        const uint32_t wbase = span * 64u + lane;
        const uint32_t p0 = wbase * 32u;
        uint32_t ww = span_word(S.bitmap[wbase], p0, from_rel, to_rel);
        while (ww) {
            const uint32_t p = p0 + (uint32_t)__ffs(ww) - 1u;
            ww &= ww - 1u;
            pend_set(S, p, (uint32_t)S.tile[p] + 3u);
        }
    }
    __syncthreads();
    // phase B
    for (uint32_t span = span0 + wv; span < span1; span += NW) {
        wave_sync<NW>();
        const uint32_t wbase = span * 64u + lane;
        const uint32_t p0 = wbase * 32u;
        const uint32_t w = span_word(S.bitmap[wbase], p0, from_rel, to_rel);
        S.bitmap[wbase] = 0; /* consumed */
        uint32_t total;
        const uint32_t pre = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        {
            uint32_t k = pre, ww = w;
            while (ww) {
                const uint32_t bit = (uint32_t)__ffs(ww) - 1u;
                ww &= ww - 1u;
                S.mpos[wv][k++] = (uint16_t)(p0 + bit);
            }
        }
        wave_sync<NW>();
        uint32_t next = 0; /* matches of the span handed out so far (wave-uniform) */
        int pending = 0;
        uint32_t p = 0, len = 0, dist = 1, chk_p = 0, chk_n = 0, idle = 0;
        int64_t src_rel = 0;
        for (;;) {
            // refill: every free lane takes the next match of the span, in order
            {
                const unsigned long long freem = __ballot(!pending);
                const uint32_t q = next + (uint32_t)__popcll(freem & lt_mask);
                if (!pending && q < total) {
                    p = S.mpos[wv][q];
                    len = (uint32_t)S.tile[p] + 3u;
                    dist = ((uint32_t)S.tile[p + 1] | ((uint32_t)S.tile[p + 2] << 8)) + 1u;
                    src_rel = (int64_t)p - (int64_t)dist;                 /* tile relative, may be < 0 */
                    const uint32_t span_len = len < dist ? len : dist;     /* distinct source bytes   */
                    const int64_t t0 = src_rel > lds_rel0 ? src_rel : lds_rel0; /* the part in the tile */
                    const int64_t t1 = src_rel + (int64_t)span_len;
                    chk_p = (uint32_t)(t0 < t1 ? t0 : 0);
                    chk_n = (uint32_t)(t0 < t1 ? t1 - t0 : 0);
                    pending = 1;
                }
                const uint32_t nfree = (uint32_t)__popcll(freem);
                next = next + nfree < total ? next + nfree : total;
            }
            if (!__any(pending)) break;
            wave_sync<NW>(); /* copies and cleared bits of the previous round are visible */
            const int ready = pending && !pend_any(S, chk_p, chk_n);
            if (!__any(ready)) {
                // NW > 1: every source still belongs to another wavefront -- poll.  (With one
                // wavefront this cannot happen.)  The bound on idle polls keeps a logic error
                // from becoming a hung GPU; it is REPORTED: the unresolved matches still hold
                // their descriptors, so the stream must not come back as good.
                if (NW == 1 || ++idle > idle_bound || S.internal_err) {
                    S.internal_err = 1;
                    break;
                }
                resolve_poll_pause();
                continue;
            }
            idle = 0;
            lds_acquire_workgroup(); /* the source bytes behind the cleared bits */
            const int src_in_lds = src_rel >= lds_rel0;
            const int simple = ready && len <= 16u && dist >= len;
            // (a) short, non-overlapping, source in the tile: by the lane itself
            copy_short_match(S, simple && src_in_lds, p, len, (uint32_t)src_rel);
            // (b) everything else (long, self-overlapping, straddling the flush point; matches
            //     whose whole source is already flushed never get here: far_copy took them):
            //     one match at a time, all 64 lanes copy
            unsigned long long gm = __ballot(ready && !(simple && src_in_lds));
            while (gm) {
                const int sl = __ffsll(gm) - 1;
                gm &= gm - 1;
                const uint32_t lp = wave_bcast_u32(p, (uint32_t)sl);
                const uint32_t ll = wave_bcast_u32(len, (uint32_t)sl);
                const uint32_t ld = wave_bcast_u32(dist, (uint32_t)sl);
                copy_match_wave(S, O, lp, ll, ld);
            }
            wave_sync<NW>(); /* the copied bytes are in LDS before their pending bits drop */
            lds_release_workgroup();
            if (ready) {
                pend_clear(S, p, len);
                pending = 0;
            }
        }
        if (S.internal_err) break; /* (set by this or another wavefront; re-read after the barrier) */
    }
    __syncthreads();
    const int err = S.internal_err != 0;
    if (err) {
        // leave the tile bookkeeping clean: nothing of this range is pending or marked any more
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < sizeof(S.pend) / 4; k += 64u * NW) S.pend[k] = 0;
        for (uint32_t k = threadIdx.x; k < sizeof(S.bitmap) / 4; k += 64u * NW) S.bitmap[k] = 0;
        if (threadIdx.x == 0) S.internal_err = 0;
        __syncthreads();
    }
    return err;
}

// Group variant of resolve_matches() for ONE wavefront per workgroup (throughput regime: other
// wavefronts of the CU fill the gaps, so the cheaper bookkeeping wins: fixed-Huffman 146.3 vs
// 142.7 GB/s, config-5 shard 158.2 vs 154.4 with the sliding window).
// Resolve, in stream order, every match whose start lies in tile-relative [from_rel, to_rel).
// Matches were left by pass 2 as {len-3, (dist-1) lo, (dist-1) hi} in their first three
// destination bytes plus a bit in S.bitmap.  Replaces the reference's copy
// (src/inflate.c:1842-1897; byte-by-byte semantics, overlap replicates).
//
// 64 matches at a time, one per lane.  A match may be copied as soon as none of its source
// bytes is still the pending destination of an earlier match (S.pend); the first pending
// match always qualifies, so every round makes progress, and ordinary data needs one or two
// rounds per group.  Sources older than the tile come from the flushed output (HBM/L2).
template <class LDS> DEV_INLINE void resolve_matches_groups(LDS &S, OutState &O, uint32_t from_rel, uint32_t to_rel)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    const uint32_t lane = lane_id();
    const int64_t lds_rel0 = O.lds_from - O.tile_base; /* tile bytes below this are not in LDS */
    for (uint32_t span = from_rel >> 11; span < ((to_rel + 2047u) >> 11); span++) {
        wave_sync<NW>();
        uint32_t wbase = span * 64u + lane;
        uint32_t w = S.bitmap[wbase];
        uint32_t p0 = wbase * 32u;
        if (p0 + 32u <= from_rel || p0 >= to_rel) w = 0;
        else {
            if (p0 < from_rel) w &= ~0u << (from_rel - p0);
            if (p0 + 32u > to_rel) w &= (1u << (to_rel - p0)) - 1u;
        }
        S.bitmap[wbase] = 0; /* consumed */
        uint32_t total;
        uint32_t pre = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        {
            uint32_t k = pre, ww = w;
            while (ww) {
                uint32_t bit = (uint32_t)__ffs(ww) - 1u;
                ww &= ww - 1u;
                S.mpos[wave_id()][k++] = (uint16_t)(p0 + bit);
            }
        }
        wave_sync<NW>();
        for (uint32_t g = 0; g < total; g += 64) {
            uint32_t q = g + lane;
            int pending = q < total;
            uint32_t p = 0, len = 0, dist = 1;
            if (pending) {
                p = S.mpos[wave_id()][q];
                len = (uint32_t)S.tile[p] + 3u;
                dist = ((uint32_t)S.tile[p + 1] | ((uint32_t)S.tile[p + 2] << 8)) + 1u;
            }
            const int64_t src_rel = (int64_t)p - (int64_t)dist;   /* tile relative, may be < 0 */
            const uint32_t span_len = len < dist ? len : dist;     /* distinct source bytes   */
            // part of the source range that lives in the LDS tile
            int64_t t0 = src_rel > lds_rel0 ? src_rel : lds_rel0;
            int64_t t1 = src_rel + (int64_t)span_len;
            const uint32_t chk_p = (uint32_t)(t0 < t1 ? t0 : 0);
            const uint32_t chk_n = (uint32_t)(t0 < t1 ? t1 - t0 : 0);
            const int src_in_lds = src_rel >= lds_rel0;
            wave_sync<NW>();
            if (pending) pend_set(S, p, len);
            wave_sync<NW>();
            for (;;) {
                if (!__any(pending)) break;
                int ready = pending && !pend_any(S, chk_p, chk_n);
                int simple = ready && len <= 16u && dist >= len;
                // (a) short, non-overlapping, source in the tile
                copy_short_match(S, simple && src_in_lds, p, len, (uint32_t)src_rel);
                // (b) everything else (long, self-overlapping, straddling the flush point; matches
                //     whose whole source is already flushed never get here: far_copy took them):
                //     one match at a time, all 64 lanes copy
                unsigned long long gm = __ballot(ready && !(simple && src_in_lds));
                while (gm) {
                    int sl = __ffsll(gm) - 1;
                    gm &= gm - 1;
                    const uint32_t lp = wave_bcast_u32(p, (uint32_t)sl);
                    const uint32_t ll = wave_bcast_u32(len, (uint32_t)sl);
                    const uint32_t ld = wave_bcast_u32(dist, (uint32_t)sl);
                    copy_match_wave(S, O, lp, ll, ld);
                }
                wave_sync<NW>();
                if (ready) {
                    pend_clear(S, p, len);
                    pending = 0;
                }
                wave_sync<NW>();
            }
        }
    }
    wave_sync<NW>();
}

// ------------------------------------------------------------------ segment scan (pass 1)
// 64 bits of the staged window starting at lp: one LDS round trip serves the literal/length
// code, its extra bits, the distance code and its extra bits (<= 48 bits in all)
struct Win64 {
    uint32_t lo, hi;
};
template <class LDS> DEV_INLINE Win64 win64(const LDS &S, uint32_t lp)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    uint32_t w = lp >> 5, sh = lp & 31u;
    uint32_t d0 = S.inwin[w], d1 = S.inwin[w + 1], d2 = S.inwin[w + 2];
    Win64 r;
    r.lo = funnel32(d1, d0, sh);
    r.hi = funnel32(d2, d1, sh);
    return r;
}

struct SegInfo {
    uint32_t end;        /* LENIENT end: window-relative bit position of the first symbol at/after seg_end */
    uint32_t strict_end; /* where strict decoding stopped (after the EOB code, ...)             */
    uint32_t nbytes;     /* output bytes of the emitting symbols before the first terminal event */
    uint32_t nsym;       /* emitting symbols (literals + matches) before it                      */
    uint32_t flag;       /* FL_* : the first terminal event, FL_CONT if none                     */
    uint32_t status;     /* DEBIG_E_* when FL_ERR                                                */
    /* checkpoint at the first symbol that starts at or after the middle of the segment: pass 2
     * splits every segment there so that all 64 lanes have work for one tile of output */
    uint32_t mid_lp, mid_nbytes, mid_nsym;
};

DEV_INLINE SegInfo seg_info_empty()
{
    SegInfo r;
    r.end = 0; r.strict_end = 0; r.nbytes = 0; r.nsym = 0; r.flag = FL_CONT; r.status = 0;
    r.mid_lp = 0; r.mid_nbytes = 0; r.mid_nsym = 0;
    return r;
}

// One symbol, every case handled (long codes, end of block, tail gate, undecodable patterns):
// the general step of pass 1.  See scan_segment for the lenient/strict contract.
template <class LDS> DEV_INLINE void scan_step_general(const LDS &S, uint32_t &lp, uint32_t &live, uint32_t &nbytes,
                                  uint32_t &nsym, SegInfo &r, int32_t tail_l)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    // Q2 tail gate (src/inflate.c:1702): stop everything once ceil(bits/8) >= in_size
    if (live && (int32_t)lp > tail_l) { r.flag = FL_TAIL; live = 0; r.strict_end = lp; }
    Win64 wb = win64(S, lp);
    uint32_t bits = wb.lo;
    uint32_t e = S.t.lit_tab[bits & S.t.mask[CODE_LIT]];
    if (ENT_LEN(e) == 0) e = huff_slow(bits, S, CODE_LIT, e);
    uint32_t l = ENT_LEN(e), kind = ENT_KIND(e), nx = ENT_EXTRA(e);
    if (l == 0) { /* no code */
        if (live) { r.flag = FL_ERR; r.status = DEBIG_E_NO_CODE; live = 0; r.strict_end = lp; }
        lp += 1;
        return;
    }
    if (kind >= 2u) { /* end of block | symbols 286/287 */
        lp += l;
        if (live) {
            r.flag = kind == 2u ? FL_EOB : FL_ERR;
            r.status = kind == 2u ? 0u : (uint32_t)DEBIG_E_LITLEN_286_287;
            live = 0;
            r.strict_end = lp;
        }
        return;
    }
    uint32_t val = ENT_VAL(e) + ((bits >> l) & ((1u << nx) - 1u)); /* literal byte or length */
    lp += l + nx;
    if (kind == 1u) {
        uint32_t bits2 = funnel32(wb.hi, wb.lo, l + nx);
        uint32_t de = S.t.dist_tab[bits2 & S.t.mask[CODE_DIST]];
        if (ENT_LEN(de) == 0) de = huff_slow(bits2, S, CODE_DIST, de);
        uint32_t ld = ENT_LEN(de);
        if (ld == 0 || (de & 0x100u)) { /* no code | distance symbol 30/31 */
            if (live) {
                r.flag = FL_ERR;
                r.status = ld == 0 ? (uint32_t)DEBIG_E_NO_CODE : (uint32_t)DEBIG_E_DIST_SYMBOL;
                live = 0;
                r.strict_end = lp;
            }
            lp += ld == 0 ? 1u : ld;
            return;
        }
        lp += ld + ENT_EXTRA(de);
        nbytes += live ? val : 0u;
    } else {
        nbytes += live;
    }
    nsym += live;
}

// Pass 1: decode from `start` until a symbol starts at or beyond seg_end (window-relative bit
// positions).  The scan is LENIENT: end-of-block, the tail gate and undecodable patterns do not
// stop it (a lane that starts at a guessed bit position is decoding garbage until it falls into
// step with the real symbol sequence, and must get there).  What a STRICT decoder would have
// seen is frozen at the first such event: for a lane whose start is the true one these frozen
// values are exactly the reference's behaviour, and lanes behind it are discarded.
//
// The loop body is straight-line for the common case (short code, literal or match): one LDS
// round trip for 64 window bits, one for the literal/length entry, one for the distance
// entry (looked up unconditionally; unused for literals), selects instead of branches.
// Anything else drops to scan_step_general for that one symbol.
//
// STOP = true is the strict probe of a short block: the scan ends at the first terminal event
// (the caller knows `start` is the true position, so nothing behind that event is needed).
template <bool STOP = false, class LDS> DEV_INLINE SegInfo scan_segment(const LDS &S, uint32_t start, uint32_t seg_end, int32_t tail_l)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    SegInfo r;
    r.flag = FL_CONT;
    r.status = 0;
    r.strict_end = start;
    uint32_t nbytes = 0, nsym = 0, live = 1; /* live: no terminal event yet */
    uint32_t lp = start;
    uint32_t flag = FL_CONT, status = 0, strict_end = start;
    const uint32_t seg_mid = seg_end - SegCfg<NW>::BITS / 2;
    uint32_t mid_lp = 0, mid_nbytes = 0, mid_nsym = 0, got_mid = 0;
    const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
    while (lp < seg_end && (!STOP || live)) {
        {
            uint32_t cross = (uint32_t)(lp >= seg_mid) & ~got_mid & 1u;
            mid_lp = cross ? lp : mid_lp;
            mid_nbytes = cross ? nbytes : mid_nbytes;
            mid_nsym = cross ? nsym : mid_nsym;
            got_mid |= cross;
        }
        Win64 wb = win64(S, lp);
        uint32_t e = S.t.lit_tab[wb.lo & lm];
        uint32_t l = ENT_LEN(e), kind = ENT_KIND(e), nx = ENT_EXTRA(e);
        uint32_t n1 = l + nx;
        uint32_t val = ENT_VAL(e) + ((wb.lo >> l) & ((1u << nx) - 1u));
        uint32_t de = S.t.dist_tab[funnel32(wb.hi, wb.lo, n1) & dm];
        uint32_t ld = ENT_LEN(de);
        uint32_t is_len = kind == 1u;
        // codes longer than the direct tables (or no code at all): the general step
        if ((l == 0) | (is_len & (ld == 0))) {
            r.flag = flag; r.status = status; r.strict_end = strict_end;
            scan_step_general(S, lp, live, nbytes, nsym, r, tail_l);
            flag = r.flag; status = r.status; strict_end = r.strict_end;
            continue;
        }
        // everything else without branches.  Terminal events (tail gate before the symbol;
        // end of block, symbols 286/287, distance symbols 30/31 after it) freeze the strict
        // view once; the lenient scan itself just keeps going.
        uint32_t gate = live & (uint32_t)((int32_t)lp > tail_l);
        flag = gate ? (uint32_t)FL_TAIL : flag;
        strict_end = gate ? lp : strict_end;
        live &= ~gate;
        uint32_t derr = is_len & ((de >> 8) & 1u);
        uint32_t term = (kind >= 2u) | derr;
        uint32_t lp_sym = lp + n1;                     /* after the literal/length code + extra */
        lp = lp_sym + (is_len ? ld + (derr ? 0u : ENT_EXTRA(de)) : 0u);
        uint32_t fire = live & term;
        flag = fire ? (kind == 2u ? (uint32_t)FL_EOB : (uint32_t)FL_ERR) : flag;
        status = fire ? (kind == 3u ? (uint32_t)DEBIG_E_LITLEN_286_287
                                    : (derr ? (uint32_t)DEBIG_E_DIST_SYMBOL : 0u)) : status;
        strict_end = fire ? lp_sym : strict_end;
        live &= ~term;
        nbytes += live ? (is_len ? val : 1u) : 0u;
        nsym += live;
    }
    r.flag = flag;
    r.status = status;
    r.strict_end = strict_end;
    r.end = lp;
    if (live) r.strict_end = lp;
    r.nbytes = nbytes;
    r.nsym = nsym;
    r.mid_lp = got_mid ? mid_lp : lp; /* no symbol starts in the second half: it is empty */
    r.mid_nbytes = got_mid ? mid_nbytes : nbytes;
    r.mid_nsym = got_mid ? mid_nsym : nsym;
    return r;
}

// Round 1 of pass 1 only has to find where each guessed trajectory ENDS (every lane is
// decoded again from its predecessor's end in round 2): positions only, no bookkeeping.
template <class LDS> DEV_INLINE uint32_t scan_positions(const LDS &S, uint32_t start, uint32_t seg_end)
{
    constexpr int NW = LDS::NW;
    (void)NW;
    uint32_t lp = start;
    const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
    while (lp < seg_end) {
        Win64 wb = win64(S, lp);
        uint32_t e = S.t.lit_tab[wb.lo & lm];
        uint32_t l = ENT_LEN(e), kind = ENT_KIND(e), nx = ENT_EXTRA(e);
        uint32_t n1 = l + nx;
        uint32_t de = S.t.dist_tab[funnel32(wb.hi, wb.lo, n1) & dm];
        uint32_t ld = ENT_LEN(de);
        uint32_t is_len = kind == 1u;
        if ((l == 0) | (is_len & (ld == 0))) { /* long code or no code: the general step */
            SegInfo dummy;
            uint32_t live = 0, nb = 0, ns = 0;
            dummy.flag = FL_CONT; dummy.status = 0; dummy.strict_end = 0;
            scan_step_general(S, lp, live, nb, ns, dummy, 0x7ffffff0);
            continue;
        }
        uint32_t derr = is_len & ((de >> 8) & 1u);
        lp += n1 + (is_len ? ld + (derr ? 0u : ENT_EXTRA(de)) : 0u);
    }
    return lp;
}

// ------------------------------------------------------------------ stored blocks
// Copy LEN bytes of a stored block (src/inflate.c:958-989) from the input (byte index src) to
// dst, by all 64*NW threads of the workgroup: destination-aligned 16 B/lane stores; the source
// is almost never aligned (5 header bytes precede it): aligned dword loads + a byte funnel,
// four rows in flight.  Input bytes at index >= in_len read as zero.
template <int NW> DEV_INLINE void stored_copy(const uint8_t *in, uint64_t in_len, int64_t src, uint8_t *dst, uint32_t len)
{
    const uint32_t tid = group_tid<NW>();
    const uint32_t ROW = 64u * NW * 16u; /* bytes one pass of the workgroup moves */
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head > len) head = len;
    if (tid < head) {
        int64_t i = src + tid;
        dst[tid] = ((uint64_t)i < in_len) ? in[i] : 0;
    }
    uint32_t body = (len - head) & ~15u;
    // fast part: every source byte of [0, fast) lies inside the input
    uint32_t fast = ((uint64_t)(src + head) + body <= in_len) ? body : 0;
    {
        const uint8_t *sbase = in + src + head;
        const uint32_t shb = (uint32_t)((uintptr_t)sbase & 3u);
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>((uintptr_t)sbase & ~(uintptr_t)3);
        uint32_t off = tid * 16u;
#ifndef DEBIG_STORED_ROWS
#define DEBIG_STORED_ROWS 4 /* 16-byte pieces in flight per lane */
#endif
        constexpr int SR = DEBIG_STORED_ROWS;
        for (; off + (uint32_t)(SR - 1) * ROW < fast; off += (uint32_t)SR * ROW) {
            uint32_t d[SR][5];
DEV_UNROLL
            for (int r = 0; r < SR; r++) {
                const uint32_t *q = s4 + ((off + ROW * (uint32_t)r) >> 2);
                d[r][0] = q[0]; d[r][1] = q[1]; d[r][2] = q[2]; d[r][3] = q[3];
                d[r][4] = shb ? q[4] : 0u;
            }
DEV_UNROLL
            for (int r = 0; r < SR; r++) {
                uint4 v;
                v.x = alignbyte32(d[r][1], d[r][0], shb);
                v.y = alignbyte32(d[r][2], d[r][1], shb);
                v.z = alignbyte32(d[r][3], d[r][2], shb);
                v.w = alignbyte32(d[r][4], d[r][3], shb);
                st_global_u4(dst + head + off + ROW * (uint32_t)r, v);
            }
        }
        for (; off < fast; off += ROW) {
            const uint32_t *q = s4 + (off >> 2);
            uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = shb ? q[4] : 0u;
            uint4 v;
            v.x = alignbyte32(d1, d0, shb);
            v.y = alignbyte32(d2, d1, shb);
            v.z = alignbyte32(d3, d2, shb);
            v.w = alignbyte32(d4, d3, shb);
            st_global_u4(dst + head + off, v);
        }
    }
    // slow part (only when LEN runs past the input: bytes beyond read as zero)
    for (uint32_t off = fast + tid * 16u; off < body; off += ROW) {
        uint32_t w4[4] = {0, 0, 0, 0};
        for (int k = 0; k < 16; k++) {
            int64_t i = src + head + off + k;
            if ((uint64_t)i < in_len) w4[k >> 2] |= (uint32_t)in[i] << (8 * (k & 3));
        }
        uint4 v;
        v.x = w4[0]; v.y = w4[1]; v.z = w4[2]; v.w = w4[3];
        st_global_u4(dst + head + off, v);
    }
    uint32_t tail = len - head - body;
    if (tid < tail) {
        int64_t i = src + head + body + tid;
        dst[head + body + tid] = ((uint64_t)i < in_len) ? in[i] : 0;
    }
}

// builds the BTYPE 1 tables once (RFC 1951 3.2.6; reference src/inflate.c:1042-1084)
// One image per table width: instantiate with the NW whose TabCfg the consumer uses (the
// kernel itself always runs as a single wavefront).  `out` receives sizeof(WaveLdsT<NW>::t) bytes.
template <int NW> __global__ void __launch_bounds__(64) debig_fixed_tables_kernel(uint32_t *out)
{
    __shared__ WaveLdsT<NW> S;
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i < 288; i += 64)
        S.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    if (lane < 32) S.lens[288 + lane] = 5; /* distance: 5 raw bits, MSB first */
    uint32_t *w = reinterpret_cast<uint32_t *>(&S.t);
    for (uint32_t k = lane; k < sizeof(S.t) / 4; k += 64) w[k] = 0;
    __syncthreads();
    build_code(S, CODE_LIT, S.lens, 288);
    build_code(S, CODE_DIST, S.lens + 288, 32);
    __syncthreads();
    for (uint32_t k = lane; k < sizeof(S.t) / 4; k += 64) out[k] = w[k];
}

// A batch may be split over two launches by stream size (debig_hip_inflate_batch_ex, mixed
// widths): class 0 = every stream, 1 = only "small" streams, 2 = only "large" ones.  Large =
// long enough that its own critical path, not the batch, decides the run time.
#define DEBIG_CLASS_ALL 0u
#define DEBIG_CLASS_SMALL 1u
#define DEBIG_CLASS_LARGE 2u
/* class 3 (DEBIG_CLASS_RETRY, inflate_split_kernel.inc): only streams the scan/LZ77 kernel pair
 * handed back (their result says DEBIG_E_RETRY) */
/* DEBIG_LARGE_IN_BYTES / DEBIG_LARGE_OUT_BYTES: include/debig_hip.h */
DEV_INLINE int stream_in_class(const debig_stream &st, uint32_t cls)
{
    if (cls == DEBIG_CLASS_ALL || cls == 3u) return 1;
    const int large = st.in_len >= DEBIG_LARGE_IN_BYTES || st.out_cap >= DEBIG_LARGE_OUT_BYTES;
    return large == (cls == DEBIG_CLASS_LARGE);
}

#ifndef DEBIG_WAVES_PER_EU
#define DEBIG_WAVES_PER_EU 2
#endif
#ifdef DEBIG_EMU
#define DEBIG_KERNEL_ATTRS
#else
#define DEBIG_KERNEL_ATTRS __attribute__((amdgpu_waves_per_eu(DEBIG_WAVES_PER_EU)))
#endif
__global__ void __launch_bounds__(64) DEBIG_KERNEL_ATTRS
debig_inflate_kernel(const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                     const debig_stream *__restrict__ streams, debig_result *results,
                     uint32_t n_streams, const uint32_t *__restrict__ fixed_tabs, uint32_t stream_class)
{
    __shared__ WaveLds S;
    const uint32_t lane = lane_id();

    for (uint32_t sid = blockIdx.x; sid < n_streams; sid += gridDim.x) {
        const debig_stream st = streams[sid];
        if (!stream_in_class(st, stream_class)) continue; /* another launch owns this stream */
        if (stream_class == 3u) { /* only what the scan / LZ77 kernels handed back */
            const uint32_t handed = results[sid].status;
            __syncthreads(); /* every lane has read it before lane 0 writes the new result */
            if (handed != 11u /* DEBIG_E_RETRY */) continue;
        }
        const uint8_t *in = in_arena + st.in_off;
        const uint64_t in_len = st.in_len;
        OutState O;
        O.out = out_arena + st.out_off;
        O.out_cap = st.out_cap;
        O.outpos = 0;
        O.lds_from = 0;
        O.tile_base = align_anchor(O.out, 0);

        PROF_DECL
        uint32_t status = DEBIG_OK, good = 0, final_set = 0;
        uint32_t n_blocks = 0, n_windows = 0, n_rounds = 0;
        int64_t end_bits = 0; /* debig_result.in_end_bits */
        int tables = 0; /* 0 none, 1 fixed tables resident in LDS, 2 dynamic */
        int64_t staged_base = 0; /* stage_window_cached state */
        int staged_valid = 0;
        int short_mode = 0; /* the previous symbol window ended inside lane 0's segment */

        // argument gates (src/inflate.c:826-844, Q1)
        if (!(st.flags & DEBIG_STREAM_NO_REF_GATES)) {
            if (st.out_cap < in_len) status = DEBIG_E_GATE_RECIPIENT_SMALL;
            else if (in_len < 5) status = DEBIG_E_GATE_INPUT_SHORT;
        }
        if (status == DEBIG_OK) {
            final_set = 1;
            for (uint32_t k = lane; k < DEBIG_T / 32 + 16; k += 64) { S.bitmap[k] = 0; S.farmap[k] = 0; }
            for (uint32_t k = lane; k < (DEBIG_T + DEBIG_TSLACK) / 32 + 2; k += 64) S.pend[k] = 0;
            __syncthreads();

            int64_t bitpos = 0;
            int more = 1;
            while (more && status == DEBIG_OK) {
                // ---- block header (wave-uniform: every lane runs the same reader)
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
                if (btype == 3) { /* reserved: the asserts-off reference skips it (Q5) */
                    bitpos = hb.pos;
                    continue;
                }
                if (btype == 0) {
                    // ---- stored block (src/inflate.c:919-989)
                    int64_t p = (hb.pos + 7) & ~(int64_t)7;
                    br_init(hb, S, p, org);
                    br_ensure(hb, S);
                    uint32_t len = br_take(hb, 16);
                    br_ensure(hb, S);
                    uint32_t nlen = br_take(hb, 16);
                    if ((len ^ nlen) != 0xffffu) { status = DEBIG_E_STORED_NLEN; break; }
                    if ((uint64_t)O.outpos + len > O.out_cap) { status = DEBIG_E_OUTPUT_FULL; break; }
                    flush_all(S, O);
                    int64_t src = hb.pos >> 3;
                    uint8_t *dst = O.out + O.outpos;
                    stored_copy<1>(in, in_len, src, dst, len);
                    wave_mem_fence();
                    O.outpos += len;
                    O.lds_from = O.outpos;
                    O.tile_base = align_anchor(O.out, O.outpos);
                    bitpos = hb.pos + 8 * (int64_t)len;
                    continue;
                }

                // ---- Huffman block: tables
                int fixed = (btype == 1);
                int need_p2 = st.p2_on && (O.outpos > st.p2_s0);
                if (fixed) {
                    if (tables != 1) {
                        // the fixed code never changes: copy the tables debig_fixed_tables_kernel
                        // built once per process (src/inflate.c:1042-1181 rebuilds them per block)
                        __syncthreads();
                        const uint32_t *src = fixed_tabs;
                        uint32_t *dstw = reinterpret_cast<uint32_t *>(&S.t);
                        for (uint32_t k = lane; k < sizeof(S.t) / 4; k += 64) dstw[k] = src[k];
                        __syncthreads();
                        tables = 1;
                    }
                } else {
                    uint32_t hlit = br_take(hb, 5) + 257u;
                    uint32_t hdist = br_take(hb, 5) + 1u;
                    uint32_t hclen = br_take(hb, 4) + 4u;
                    if (lane < 19) S.lens[lane] = 0;
                    __syncthreads();
                    read_cl_lens(S, hb, org, hclen);
                    __syncthreads();
                    if (lane < 19) S.cl_len[lane] = S.lens[lane];
                    tables = 2;
                    if (!build_code(S, CODE_CL, S.lens, 19, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES))) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                    if (need_p2 && lane < 19) { /* table image for the aliasing replay */
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
                    __syncthreads();
                    // code lengths of the two alphabets (src/inflate.c:1416-1520), wave-uniform
                    const uint32_t total = hlit + hdist;
                    const int bad = decode_code_lengths(S, hb, org, total);
                    if (bad) { status = DEBIG_E_NO_CODE; break; }
                    __syncthreads();
                    if (!build_code(S, CODE_LIT, S.lens, hlit, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES))) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                    if (!build_code(S, CODE_DIST, S.lens + hlit, hdist, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES))) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                }
                if (need_p2) {
                    // decode_png aliasing replay (SURVEY.md Appendix C): the reference's first
                    // scratch table overwrites already decoded stream bytes [s0, outpos)
                    flush_all(S, O);
                    int64_t end = O.outpos < (int64_t)st.p2_est ? O.outpos : (int64_t)st.p2_est;
                    int64_t s_lo = st.p2_s0 > 0 ? st.p2_s0 : 0;
                    uint32_t nent = fixed ? 288u : 19u;
                    for (int64_t s = s_lo + lane; s < end; s += 64) {
                        uint64_t t = (uint64_t)(s - st.p2_s0);
                        uint64_t e = t >> 4;
                        uint32_t k = (uint32_t)(t & 15u);
                        if (e >= nent) { O.out[s] = 0; continue; }
                        if (k >= 14) continue;
                        uint32_t code, used, l;
                        if (fixed) {
                            uint32_t ei = (uint32_t)e;
                            used = 1;
                            if (ei < 144) { l = 8; code = 48 + ei; }
                            else if (ei < 256) { l = 9; code = 400 + (ei - 144); }
                            else if (ei < 280) { l = 7; code = ei - 256; }
                            else { l = 8; code = 192 + (ei - 280); }
                        } else {
                            code = S.cl_code[e]; used = S.cl_used[e]; l = S.cl_len[e];
                        }
                        uint32_t word = k < 4 ? code : k < 8 ? (uint32_t)e : k < 12 ? used : l;
                        O.out[s] = (uint8_t)(word >> (8 * (k & 3u)));
                    }
                    wave_mem_fence();
                    __syncthreads();
                }
                bitpos = hb.pos;
                PROF_END(5);

                // ---- symbol windows
                int block_done = 0;
                while (!block_done && status == DEBIG_OK) {
                    n_windows++;
                    SegInfo si = seg_info_empty();
                    uint32_t start = 0, first_term = 64;
                    int probe_hit = 0;
                    if (short_mode) {
                        // Short blocks: the previous window ended inside its first segment, so
                        // this one probably does too.  Lane 0 alone decodes strictly from the
                        // true position and stops at the first terminal event; if there is one
                        // within a segment's length, the speculative rounds are not needed.
                        PROF_BEGIN();
                        wbase = stage_window_cached(S, in, in_len, bitpos >> 3, DEBIG_PROBE_NEED, 0, staged_base, staged_valid);
                        org = 8 * wbase;
                        PROF_END(0);
                        PROF_BEGIN();
                        int64_t ptl = 8 * ((int64_t)in_len - 1) - org;
                        const int32_t ptail = ptl < -1 ? -1 : (ptl > 0x7ffffff0 ? 0x7ffffff0 : (int32_t)ptl);
                        start = (uint32_t)(bitpos - org);
                        if (lane == 0) si = scan_segment<true>(S, start, start + SEG_BITS, ptail);
                        n_rounds++;
                        probe_hit = __shfl(si.flag, 0) != FL_CONT;
                        if (probe_hit) first_term = 0;
                        else { short_mode = 0; si = seg_info_empty(); }
                        PROF_END(1);
                    }
                    if (!probe_hit) {
                    PROF_BEGIN();
                    wbase = stage_window_cached(S, in, in_len, bitpos >> 3, WIN_BYTES + 16u, 1, staged_base, staged_valid);
                    PROF_END(0);
                    PROF_BEGIN();
                    org = 8 * wbase;
                    // pass 1: speculative segment scan until the start/end chain is consistent
                    // (window-relative bit positions: bit 0 = first bit of S.inwin)
                    const uint32_t seg_lo = lane * SEG_BITS;
                    const uint32_t seg_end = seg_lo + SEG_BITS;
                    start = (lane == 0) ? (uint32_t)(bitpos - org) : seg_lo;
                    int64_t tl = 8 * ((int64_t)in_len - 1) - org;
                    const int32_t tail_l = tl < -1 ? -1 : (tl > 0x7ffffff0 ? 0x7ffffff0 : (int32_t)tl);
                    int dirty = 1;
                    si.end = start; si.strict_end = start; si.nbytes = 0; si.nsym = 0;
                    si.flag = FL_CONT; si.status = 0;
                    first_term = 64;
                    const uint32_t npos = fixed ? DEBIG_POS_ROUNDS_FIXED : DEBIG_POS_ROUNDS_DYNAMIC;
                    for (uint32_t round = 0; round < 70 + npos; round++) {
                        // the first npos rounds only chase positions (cheap); then
                        // everyone scans in full once (nobody has counts yet), then only lanes
                        // whose start moved
                        if (round < npos) { if (dirty) si.end = scan_positions(S, start, seg_end); }
                        else if (dirty) si = scan_segment(S, start, seg_end, tail_l);
                        dirty = round == npos - 1;
                        n_rounds++;
                        uint32_t prev_end = __shfl_up(si.end, 1);
                        unsigned long long cont = __ballot(si.flag == FL_CONT);
                        first_term = (~cont == 0ull) ? 64u : (uint32_t)(__ffsll(~cont) - 1);
                        // every lane follows its predecessor (lanes behind a terminal event keep
                        // converging in the background); only lanes up to it must be settled
                        if (lane > 0 && start != prev_end) {
                            start = prev_end;
                            dirty = 1;
                        }
                        if (round >= npos && !__any(dirty && lane <= first_term)) break;
                    }
                    PROF_END(1);
                    short_mode = first_term == 0;
                    } /* !probe_hit */
                    uint32_t last = first_term < 64u ? first_term : 63u;
                    int used = lane <= last;
                    uint32_t wflag = __shfl(si.flag, last);
                    uint32_t wstatus = __shfl(si.status, last);
                    int64_t wend = org + (int64_t)__shfl(si.strict_end, last);

                    // pass 2: offsets by prefix sum, then decode + emit through the LDS tile
                    uint32_t nbytes = used ? si.nbytes : 0u;
                    uint32_t wtotal;
                    uint32_t pre = wave_excl_scan_u32(nbytes, &wtotal);
                    const int64_t w_out0 = O.outpos;
                    const int64_t w_end = w_out0 + (int64_t)wtotal;
                    const int64_t my_o = w_out0 + (int64_t)pre; /* output offset of my segment */
                    uint32_t lane_err = 0;
                    int64_t lane_err_pos = 0;
                    // Two batches of 64 work items.  An item is HALF a segment (split at the
                    // mid-point checkpoint of pass 1): lane j of batch b decodes half (j & 1) of
                    // segment 32 b + j / 2, so one batch produces about one tile of output with
                    // every lane busy, in stream order.
                    for (uint32_t batch = 0; batch < 2 && status == DEBIG_OK; batch++) {
                        const int sl = (int)(32u * batch + (lane >> 1));
                        const uint32_t half = lane & 1u;
                        const uint32_t s_start = __shfl(start, sl);
                        const uint32_t s_mid = __shfl(si.mid_lp, sl);
                        const uint32_t s_nsym = __shfl(si.nsym, sl);
                        const uint32_t s_mnsym = __shfl(si.mid_nsym, sl);
                        const uint32_t s_mnb = __shfl(si.mid_nbytes, sl);
                        const int64_t s_o = __shfl(my_o, sl);
                        const int s_used = __shfl(used, sl);
                        int64_t w_out1 = batch == 0 ? __shfl(my_o, 32) : w_end; /* end of this batch's output */
                        int64_t oc = s_o + (half ? (int64_t)s_mnb : 0);
                        uint32_t remaining = s_used ? (half ? s_nsym - s_mnsym : s_mnsym) : 0u;
                        uint32_t lp = half ? s_mid : s_start;
                        for (;;) {
                            int64_t lim = O.tile_base + DEBIG_T;
                            PROF_BEGIN();
                            {
                            // the hot loop works on 32-bit tile-relative positions
                            uint32_t rel = (uint32_t)(oc - O.tile_base);       /* < T + 258 or beyond */
                            const int64_t room = (int64_t)O.out_cap - O.tile_base;
                            const uint32_t cap_rel = room > 0x7fffffff ? 0x7fffffffu : (room < 0 ? 0u : (uint32_t)room);
                            // a distance is "too far" only near the start of the stream
                            const int32_t tb32 = O.tile_base > 70000 ? 70000 : (int32_t)O.tile_base;
                            const uint32_t lds_rel = (uint32_t)(O.lds_from - O.tile_base);
                            const int64_t rel_lim64 = lim - O.tile_base; /* == T */
                            const uint32_t rel_lim = (oc - O.tile_base) >= rel_lim64 ? 0u : (uint32_t)rel_lim64;
                            const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
                            while (remaining && rel < rel_lim) {
                                // straight-line decode of one symbol (every symbol here is known to
                                // be decodable: pass 1 counted it strictly)
                                Win64 wb = win64(S, lp);
                                uint32_t e = S.t.lit_tab[wb.lo & lm];
                                if (ENT_LEN(e) == 0) e = huff_slow(wb.lo, S, CODE_LIT, e);
                                const uint32_t l = ENT_LEN(e), nx = ENT_EXTRA(e), n1 = l + nx;
                                const uint32_t val = ENT_VAL(e) + ((wb.lo >> l) & ((1u << nx) - 1u));
                                const uint32_t is_len = ENT_KIND(e) == 1u;
                                const uint32_t bits2 = funnel32(wb.hi, wb.lo, n1);
                                uint32_t de = S.t.dist_tab[bits2 & dm];
                                if (is_len && ENT_LEN(de) == 0) de = huff_slow(bits2, S, CODE_DIST, de);
                                const uint32_t ld = ENT_LEN(de), dx = ENT_EXTRA(de);
                                const uint32_t dist = ENT_VAL(de) + ((bits2 >> ld) & ((1u << dx) - 1u));
                                const uint32_t outlen = is_len ? val : 1u;
                                remaining--;
                                // rare: output would exceed recipient_size | distance beyond the
                                // start of the output (src/inflate.c:1843)
                                const uint32_t too_far = is_len & (uint32_t)((int32_t)dist > tb32 + (int32_t)rel);
                                const uint32_t full = (uint32_t)(rel + outlen > cap_rel);
                                if (too_far | full) {
                                    lane_err = too_far ? (uint32_t)DEBIG_E_DIST_TOO_FAR : (uint32_t)DEBIG_E_OUTPUT_FULL;
                                    lane_err_pos = O.tile_base + (int64_t)rel;
                                    remaining = 0;
                                    break;
                                }
                                S.tile[rel] = (uint8_t)(is_len ? val - 3u : val);
                                if (is_len) {
                                    S.tile[rel + 1] = (uint8_t)((dist - 1u) & 0xffu);
                                    S.tile[rel + 2] = (uint8_t)((dist - 1u) >> 8);
                                    // whole source already flushed? then it has no ordering constraints
                                    uint32_t *map = ((int32_t)(rel + val) - (int32_t)dist <= (int32_t)lds_rel) ? S.farmap : S.bitmap;
                                    atomicOr(&map[rel >> 5], 1u << (rel & 31u));
                                }
                                lp += n1 + (is_len ? ld + dx : 0u);
                                rel += outlen;
                            }
                            // lanes that have not reached this tile keep their position
                            if ((oc - O.tile_base) < rel_lim64) oc = O.tile_base + (int64_t)rel;
                            }
                            PROF_END(2);
                            // an error truncates the window's output at the failing token
                            unsigned long long em = __ballot(lane_err != 0);
                            if (em) {
                                int el = __ffsll(em) - 1;
                                uint32_t es = __shfl(lane_err, el);
                                int64_t ep = __shfl(lane_err_pos, el);
                                if (status == DEBIG_OK) { status = es; w_out1 = ep; }
                                remaining = 0; /* later lanes only need to stay memory-safe: stop them */
                            }
                            int64_t upto = w_out1 < lim ? w_out1 : lim;
                            uint32_t from_rel = (uint32_t)(O.outpos - O.tile_base);
                            uint32_t to_rel = (uint32_t)(upto - O.tile_base);
                            if (status != DEBIG_OK) {
                                // drop match marks at or beyond the failing position
                                __syncthreads();
                                far_copy(S, O, from_rel, to_rel);
                                resolve_matches_groups(S, O, from_rel, to_rel);
                                for (uint32_t k = lane; k < DEBIG_T / 32 + 16; k += 64) { S.bitmap[k] = 0; S.farmap[k] = 0; }
                                __syncthreads();
                                O.outpos = upto;
                                break;
                            }
                            PROF_BEGIN();
                            far_copy(S, O, from_rel, to_rel);
                            PROF_END(7);
                            PROF_BEGIN();
                            resolve_matches_groups(S, O, from_rel, to_rel);
                            PROF_END(3);
                            if (w_out1 >= lim) {
                                // tile full: the last match may run up to 257 bytes into the slack
                                int64_t min_oc = oc;
                                {
                                    // smallest write cursor among lanes that still have work, else w_out1
                                    int64_t c = remaining ? oc : w_out1;
                                    for (uint32_t d = 32; d >= 1; d >>= 1) {
                                        int64_t o2 = __shfl_xor(c, (int)d);
                                        c = o2 < c ? o2 : c;
                                    }
                                    min_oc = c < w_out1 ? c : w_out1;
                                }
                                int64_t carry_end = min_oc > lim ? min_oc : lim; /* resolved up to here */
                                PROF_BEGIN();
                                flush_range(S, O, O.lds_from, lim);
                                PROF_END(4);
                                uint32_t carry = (uint32_t)(carry_end - lim);
                                uint8_t cv[5];
DEV_UNROLL
                                for (uint32_t it = 0; it < 5; it++) {
                                    uint32_t k = it * 64u + lane;
                                    if (k < carry) cv[it] = S.tile[DEBIG_T + k];
                                }
                                __syncthreads();
DEV_UNROLL
                                for (uint32_t it = 0; it < 5; it++) {
                                    uint32_t k = it * 64u + lane;
                                    if (k < carry) S.tile[k] = cv[it];
                                }
                                __syncthreads();
                                O.tile_base = lim;
                                O.lds_from = lim;
                                O.outpos = carry_end;
                                if (!__any(remaining != 0)) {
                                    O.outpos = w_out1;
                                    break;
                                }
                            } else {
                                O.outpos = w_out1;
                                break;
                            }
                        }
                    } /* batch */
                    if (status != DEBIG_OK) break;
                    bitpos = wend;
                    if (wflag == FL_EOB) block_done = 1;
                    else if (wflag == FL_TAIL) { block_done = 1; more = 0; }
                    else if (wflag == FL_ERR) { status = wstatus; }
                }
            }
            end_bits = bitpos;
            flush_all(S, O);
            if (status == DEBIG_OK) good = 1;
        }
        if (lane == 0) {
            debig_result r;
            r.final_size = (uint64_t)O.outpos;
            r.good = good;
            r.status = status;
            r.final_set = final_set;
            r.n_blocks = n_blocks;
            r.n_windows = n_windows;
            r.n_rounds = n_rounds;
            r.in_end_bits = (uint64_t)end_bits;
            PROF_STORE(r);
            results[sid] = r;
        }
        __syncthreads();
    }
}
