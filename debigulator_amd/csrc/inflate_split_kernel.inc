// inflate_split_kernel.inc -- the throughput path: inflate in two halves, both run by the wavefront
// that owns the stream (debig_scanlz_kernel, one wavefront per stream).
//
//   scan half   (scan_body)  block headers, tables, the speculative segment scan of inflate_kernel.inc
//                            (pass 1) -- and nothing else.  Once a window's start/end chain is settled
//                            every lane has already decoded its segment's symbols: they are kept, as
//                            32-bit TOKENS in HBM, one row of 64 tokens per symbol index (lane L's k-th
//                            symbol at row k, column L: the 64 lanes store one coalesced 256-byte row
//                            per loop iteration).  Stored blocks are copied straight to the recipient here.
//   LZ77 half   (lz_body)    reads the token rows back (coalesced, several rows in flight: no table
//                            look-ups, no bit reader, no dependent LDS round trips), places literals and
//                            match descriptors in an 8 KiB LDS tile, resolves the LZ77 matches with the
//                            far/near machinery of inflate_kernel.inc and flushes the tile with 16-byte
//                            stores.
//
// Why two halves (measured on the one-pass version, profiles/r01_*): every phase of the one-pass
// kernel was latency bound at 2 wavefronts per SIMD -- 219 VGPRs and 20 KB of LDS per wavefront,
// the union of what the phases need -- and every symbol was decoded about 4 times (2 position
// rounds, 1 full round, 1 emit pass).  Split, the emit pass becomes a replay of tokens.  The price
// is HBM traffic (tokens are written and read once: about 1.5 x D each way) on a path that was
// using 7 % of the HBM bandwidth.  (Round 2 ran the halves as two kernels; why they are fused now
// is said above debig_scanlz_kernel.)
//
// What it replaces in the reference: src/inflate.c:786-1965, same observable behaviour as
// debig_inflate_kernel (the two share every helper); streams that do not fit their share of the
// token workspace are handed to debig_inflate_kernel (DEBIG_CLASS_RETRY).

/* DEBIG_E_RETRY (include/debig_hip.h): not decoded by the split path, debig_inflate_kernel takes it */
#define DEBIG_CLASS_RETRY 3u

// ---- workspace (one allocation, carved by debig_split_plan_kernel in proportion to in_len)
struct debig_ws_slot { /* 64 bytes; one per stream (one per chunk task in the chunked path) */
    uint64_t row0;  /* first 256-byte token row of the stream */
    uint32_t rows;  /* rows it may use */
    uint32_t recs;  /* records it may use */
    uint64_t rec0;  /* first record of the stream */
    uint32_t state; /* written by the scan kernel: DEBIG_OK or DEBIG_E_RETRY */
    uint32_t flags; /* chunked path, written by the scan kernel: SLOT_* */
    /* chunked path (inflate_chunk_kernel.inc): what the scan of a chunk found */
    uint64_t out_total; /* bytes the chunk's tokens and stored blocks produce */
    uint64_t end_bit;   /* bit position where its scan stopped */
    uint32_t n_blocks, n_windows, n_rounds, pad;
};
#define SLOT_MATCHED 1u /* the scan stopped exactly on the next chunk's start (or on the final block's end) */
#define SLOT_FINAL 2u   /* it consumed the stream's final block */
struct debig_ws_rec { /* 32 bytes */
    uint32_t kind;
    uint32_t row; /* stream-relative row of the record's first row */
    uint32_t a, b;
    uint64_t c, d;
};
enum {
    REC_WIN = 1,    /* symbol window: row = counts row {nsym | nbytes << 10} per lane, token rows follow;
                       a = lanes used | flag << 8, b = status of a FL_ERR window, c = output bytes */
    REC_STORED = 2, /* stored block, already copied by the scan kernel: c = LEN */
    REC_P2 = 3,     /* decode_png aliasing replay at a Huffman block header: a = fixed?, row = table image */
    REC_END = 4     /* a = status, b = n_blocks, c = in_end_bits, d = n_windows | n_rounds << 32, row = final_set */
};
#define TOK_MATCH 0x80000000u /* match: [14:0] distance - 1, [23:16] length - 3; literal: [7:0] */

// Carve the workspace: stream i gets floor(0.999 * total * w_i / W) rows and records, w_i =
// in_len + 2048.  One workgroup (1024 threads on the GPU; any power of two up to that: the CPU
// emulator uses 64); contiguous chunks of streams per thread; the three block-wide sums are
// log-step scans in LDS.
DEV_INLINE uint64_t plan_shfl_up_u64(uint64_t x, uint32_t d)
{
    const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// exclusive prefix sum over the workgroup (blockDim.x = 64 .. 1024, a multiple of 64), *total = the
// sum: shuffles inside the wavefronts, one wavefront over their totals -- three barriers
DEV_INLINE uint64_t plan_block_scan(uint64_t *buf, uint32_t t, uint64_t v, uint64_t *total)
{
    const uint32_t lane = t & 63u, wv = t >> 6, nw = blockDim.x >> 6;
    uint64_t x = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t y = plan_shfl_up_u64(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63u) buf[wv] = x;
    __syncthreads();
    if (wv == 0) {
        uint64_t w = lane < nw ? buf[lane] : 0;
        for (uint32_t d = 1; d < 16u; d <<= 1) {
            const uint64_t y = plan_shfl_up_u64(w, d);
            if (lane >= d) w += y;
        }
        buf[32u + lane] = w; /* inclusive over the wavefront totals */
    }
    __syncthreads();
    const uint64_t base = wv ? buf[32u + wv - 1u] : 0;
    *total = buf[32u + nw - 1u];
    __syncthreads();
    return base + x - v; /* exclusive */
}
// weight(i): bytes of compressed input unit i stands for (0: the unit gets nothing)
// FULL: write the whole 64-byte slot (chunk tasks read its second half); the scan / LZ77 pair only
// uses the first 32 bytes, and this one-workgroup kernel is bound by the line operations of its CU
struct __attribute__((aligned(16))) debig_ws_slot_head { /* the first 32 bytes of debig_ws_slot */
    uint64_t row0;
    uint32_t rows, recs;
    uint64_t rec0;
    uint32_t state, flags;
};
template <bool FULL, class WEIGHT>
DEV_INLINE void plan_carve(uint64_t *buf, const WEIGHT &weight, uint32_t n, debig_ws_slot *__restrict__ slots,
                           uint64_t total_rows, uint64_t total_recs)
{
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + blockDim.x - 1u) / blockDim.x;
    const uint32_t lo = t * chunk < n ? t * chunk : n;
    const uint32_t hi = lo + chunk < n ? lo + chunk : n;
    // The first 16 units of a thread are handled in fully unrolled loops: their weights are read
    // ONCE, all loads in flight together, and stay in registers through the three passes (a batch of
    // 16384 streams is 16 per thread); what lies beyond goes through plain loops that re-read.
    constexpr uint32_t KEEP = 16;
    uint64_t wk[KEEP];
    DEV_UNROLL
    for (uint32_t k = 0; k < KEEP; k++) wk[k] = lo + k < hi ? weight(lo + k) : 0;
    uint64_t w = 0;
    DEV_UNROLL
    for (uint32_t k = 0; k < KEEP; k++) w += wk[k];
    for (uint32_t i = lo + KEEP; i < hi; i++) w += weight(i);
    uint64_t W;
    (void)plan_block_scan(buf, t, w, &W);
    if (W == 0) W = 1;
    // unit i gets floor(w_i * K / 2^32), K = 0.999 * total / W in 32.32 fixed point: two doubles per
    // kernel, a 128-bit product per unit (a double -> integer conversion per unit and resource was most
    // of this kernel's 30 us)
    const uint64_t Kr = (uint64_t)(0.999 * (double)total_rows / (double)W * 4294967296.0);
    const uint64_t Kq = (uint64_t)(0.999 * (double)total_recs / (double)W * 4294967296.0);
#define PLAN_SHARE(wi, K) ((__umul64hi((wi), (K)) << 32) | (((wi) * (K)) >> 32))
    /* record shares in multiples of 4 records = 128 bytes: no cache line holds records of two streams (the
     * fused scan + LZ77 kernel reads back what the same wavefront wrote, with ordinary loads) */
#define PLAN_SHARE_Q(wi) (PLAN_SHARE((wi), Kq) & ~3ull)
    uint64_t r = 0, q = 0;
    for (uint32_t k = 0; k < KEEP; k++) { /* left rolled (measured: 19 us rolled, 32 us unrolled) */
        if (k >= chunk) break; /* workgroup-uniform */
        r += PLAN_SHARE(wk[k], Kr);
        q += PLAN_SHARE_Q(wk[k]);
    }
    for (uint32_t i = lo + KEEP; i < hi; i++) {
        const uint64_t wi = weight(i);
        r += PLAN_SHARE(wi, Kr);
        q += PLAN_SHARE_Q(wi);
    }
    uint64_t dummy;
    uint64_t r0 = plan_block_scan(buf, t, r, &dummy);
    uint64_t q0 = plan_block_scan(buf, t, q, &dummy);
#define PLAN_SLOT(i, wi)                                                                         \
    do {                                                                                         \
        const uint64_t wv_ = (wi);                                                               \
        const uint64_t ri = PLAN_SHARE(wv_, Kr);                                                 \
        const uint64_t qi = PLAN_SHARE_Q(wv_);                                                    \
        debig_ws_slot s;                                                                         \
        s.row0 = r0;                                                                             \
        s.rows = ri > 0xffffffffull ? 0xffffffffu : (uint32_t)ri;                                \
        s.rec0 = q0;                                                                             \
        s.recs = qi > 0xffffffffull ? 0xffffffffu : (uint32_t)qi;                                \
        s.state = DEBIG_E_RETRY; /* until the scan kernel says otherwise */                      \
        s.flags = 0; s.out_total = 0; s.end_bit = 0; s.n_blocks = 0; s.n_windows = 0; s.n_rounds = 0; s.pad = 0; \
        if (FULL) slots[i] = s;                                                                  \
        else {                                                                                   \
            debig_ws_slot_head hd;                                                               \
            hd.row0 = s.row0; hd.rows = s.rows; hd.recs = s.recs; hd.rec0 = s.rec0; hd.state = s.state; hd.flags = 0; \
            *reinterpret_cast<debig_ws_slot_head *>(&slots[i]) = hd;                             \
        }                                                                                        \
        r0 += ri;                                                                                \
        q0 += qi;                                                                                \
    } while (0)
    for (uint32_t k = 0; k < KEEP; k++) { /* left rolled, as above */
        if (k >= chunk) break; /* workgroup-uniform */
        if (lo + k < hi) PLAN_SLOT(lo + k, wk[k]);
    }
    for (uint32_t i = lo + KEEP; i < hi; i++) PLAN_SLOT(i, weight(i));
#undef PLAN_SLOT
#undef PLAN_SHARE_Q
#undef PLAN_SHARE
}
// work queue of the fused kernel: SPLIT_QUEUE_WORDS words right behind the n slots (the host reserves
// them: split_slots_bytes).  [0] streams handed out beyond the first gridDim.x, [1] workgroups finished
#define SPLIT_QUEUE_WORDS 4u
DEV_INLINE uint32_t *split_queue(debig_ws_slot *slots, uint32_t n) { return reinterpret_cast<uint32_t *>(slots + n); }
// DISPATCH ORDER, n words behind the queue (the host reserves them: split_slots_bytes): workgroup b of
// debig_scanlz_kernel / debig_strand_kernel takes stream perm[b].  One workgroup per stream is dealt to the shader
// engines by INDEX, whatever it costs: 4096 Huffman streams alternating with 4096 stored ones put every expensive
// stream on the same half of the chip (1.59 ms instead of 0.90: bench.py roofline_interleaved, round 4).  The plan
// kernel therefore lists the streams that look expensive first -- everything but streams whose recipient is no
// larger than their input + 64 bytes, i.e. stored / incompressible data, which is a copy -- each class in the
// caller's order (a stable partition: one more block-wide prefix sum in a kernel that already does three).
DEV_INLINE uint32_t *split_perm(debig_ws_slot *slots, uint32_t n) { return split_queue(slots, n) + SPLIT_QUEUE_WORDS; }
DEV_INLINE const uint32_t *split_perm(const debig_ws_slot *slots, uint32_t n)
{
    return reinterpret_cast<const uint32_t *>(slots + n) + SPLIT_QUEUE_WORDS;
}
DEV_INLINE int split_stream_is_cheap(const debig_stream &st) { return st.out_cap <= st.in_len + 64u; }
struct PlanStreamWeight {
    const debig_stream *streams;
    // the compressed bytes, plus a term for the recipient: a highly compressible stream (image rows of flat colour: 30 KB for
    // 4 MB, a block every few hundred bytes) has a window -- info rows, at least one unit row -- per block, many times what
    // its input length suggests; with shares by input length alone such streams went to the one-kernel path (config 3:
    // 69 instead of 39 ms).  Capped by the input, so that a caller's generous recipient_size cannot starve the others.
    // A SHORT stream of one- and two-bit codes (a run of one byte: 60 KB from 50 bytes) is the other end of the same matter:
    // one or two lanes decode all of it, and the symbols of a window's busiest lane take a token ROW each -- about
    // out_cap / 258 rows, up to the 272 two-bit symbols of a 68-byte lane segment, whatever the input length says (4 in_len is
    // a few hundred units there).  A unit is worth 12 bytes = 1 / 22.8 row (debig_hip_inflate_workspace_bytes_io), so below
    // PLAN_SHORT_IN_BYTES of input the recipient counts as out_cap / 16, at most PLAN_SHORT_UNITS: with the 2048 of every
    // stream that is 92 + out_cap / 364 rows up to 64 KiB of recipient and 281 rows beyond.  From PLAN_SHORT_IN_BYTES on
    // in_len + 4 in_len + 2048 is that much by itself.
#define PLAN_SHORT_IN_BYTES 1024u
#define PLAN_SHORT_UNITS 4352u
    DEV_MEMBER_INLINE uint64_t operator()(uint32_t i) const
    {
        const uint64_t il = streams[i].in_len, cap = streams[i].out_cap, oc = cap >> 6;
        uint64_t t = oc < 4u * il ? oc : 4u * il;
        if (il < PLAN_SHORT_IN_BYTES) {
            const uint64_t s = (cap >> 4) < PLAN_SHORT_UNITS ? (cap >> 4) : PLAN_SHORT_UNITS;
            t = t > s ? t : s;
        }
        return il + t + 2048u;
    }
};
__global__ void __launch_bounds__(1024)
debig_split_plan_kernel(const debig_stream *__restrict__ streams, uint32_t n, debig_ws_slot *__restrict__ slots,
                        uint64_t total_rows, uint64_t total_recs)
{
    __shared__ uint64_t buf[1024];
    PlanStreamWeight w;
    w.streams = streams;
    plan_carve<false>(buf, w, n, slots, total_rows, total_recs);
    // the work queue of debig_scanlz_kernel (behind the slots): every launch leaves it zeroed again
    if (threadIdx.x < SPLIT_QUEUE_WORDS) split_queue(slots, n)[threadIdx.x] = 0;
    // dispatch order: expensive-looking streams first, each class in the caller's order
    {
        const uint32_t t = threadIdx.x;
        const uint32_t chunk = (n + blockDim.x - 1u) / blockDim.x;
        const uint32_t lo = t * chunk < n ? t * chunk : n;
        const uint32_t hi = lo + chunk < n ? lo + chunk : n;
        uint64_t mine = 0;
        for (uint32_t i = lo; i < hi; i++) mine += (uint64_t)!split_stream_is_cheap(streams[i]);
        uint64_t total_e;
        __syncthreads();
        uint64_t rank_e = plan_block_scan(buf, t, mine, &total_e); /* expensive streams in front of my chunk */
        uint32_t *perm = split_perm(slots, n);
        for (uint32_t i = lo; i < hi; i++) {
            if (!split_stream_is_cheap(streams[i])) perm[rank_e++] = i;
            else perm[(uint32_t)total_e + (i - (uint32_t)rank_e)] = i;
        }
    }
}

// ------------------------------------------------------------------ scan half
// 16-bit table entries: the scan kernel's tables take 3 KB instead of 6 (with the 4.4 KB input
// window: 9.4 KB of LDS per wavefront -> 16 wavefronts per CU).
//   litlen: [3:0] code length l | [6:4] x = extra-bit count | [7] length code | [15:8] v
//           literal: x = 0, v = the byte;  length code: v = base - 3 (RFC 1951 3.2.5: 3..258 ->
//           0..255), so the token's length field is v + extra bits.
//           l = 0 marks everything the hot loops do not handle: 0 = no code starts with these bits;
//           a SPECIAL short symbol: [6:4] 1 = end of block, 3 = symbols 286/287 (bit 4 set), [11:8]
//           its code length; a LINK to a second-level table (long codes) or the SLOW mark, below.
//   dist  : [4:0] code length + extra-bit count (0 = not for the hot loops) | [8:5] extra-bit count |
//           [10:9] m.  Symbol > 29: 0x800 | code length << 12 (low byte zero).
//   both  : LINK = [4:0] 0 | [7:5] k (1..6 index bits) | [15:8] base: the symbol is
//           sub_tab[base + next k bits];  SLOW = 0x0100: canonical probe (second-level tables full)
//           distance - 1 = (m << extra) + extra bits   (symbols 0..3: m = symbol, no extra bits;
//           symbol s >= 4: extra = s/2 - 1, m = 2 + (s & 1))
struct Fmt16 {
    typedef uint16_t T;
    static constexpr uint32_t CL_SHIFT = 8;
    DEV_MEMBER uint32_t lit(uint32_t sym, uint32_t l)
    {
        if (sym < 256u) return l | (sym << 8);
        if (sym == 256u) return (1u << 4) | (l << 8);
        if (sym > 285u) return (3u << 4) | (l << 8);
        uint32_t lc = sym - 257u, ex, base;
        if (lc < 8u) { ex = 0; base = 3u + lc; }
        else if (lc == 28u) { ex = 0; base = 258u; }
        else { ex = (lc >> 2) - 1u; base = ((4u + (lc & 3u)) << ex) + 3u; }
        return l | (ex << 4) | 0x80u | ((base - 3u) << 8);
    }
    DEV_MEMBER uint32_t dist(uint32_t sym, uint32_t l)
    {
        if (sym > 29u) return 0x800u | (l << 12);
        if (sym < 4u) return l | (sym << 9);
        const uint32_t ex = (sym >> 1) - 1u;
        return (l + ex) | (ex << 5) | ((2u + (sym & 1u)) << 9);
    }
    DEV_MEMBER uint32_t cl(uint32_t sym, uint32_t l) { return l | (sym << 8); }
    static constexpr uint32_t MAX_LINK_K = 6;
    DEV_MEMBER uint32_t link(uint32_t base, uint32_t k) { return (k << 5) | (base << 8); }
    DEV_MEMBER uint32_t slowmark() { return 0x0100u; }
    DEV_MEMBER int is_link(uint32_t e) { return (e & 0x1fu) == 0 && (e & 0xe0u) != 0; }
    DEV_MEMBER uint32_t link_k(uint32_t e) { return (e >> 5) & 7u; }
    DEV_MEMBER uint32_t link_base(uint32_t e) { return e >> 8; }
    DEV_MEMBER int is_slow(uint32_t e) { return e == 0x0100u; }
};
#define E16_LEN(e) ((e) & 15u)
#define E16_X(e) (((e) >> 4) & 7u)
#define E16_ISLEN(e) (((e) >> 7) & 1u)
#define E16_V(e) ((e) >> 8)
#define E16_LENMASK(e) ((uint32_t)((int32_t)((e) << 24) >> 31)) /* bit 7 spread: 0 or ~0 */
#define E16_SPECIAL_LEN(e) (((e) >> 8) & 15u)
#define D16_TOTAL(e) ((e) & 31u)
#define D16_EXTRA(e) (((e) >> 5) & 15u)
#define D16_M(e) (((e) >> 9) & 3u)
#define D16_BAD(e) (((e) >> 11) & 1u)

DEV_INLINE uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

struct __attribute__((aligned(16))) ScanLds {
    static constexpr int NW = 1;
    static constexpr uint32_t WIN_B = SegCfg<1>::WIN;
    typedef Fmt16 Fmt;
    uint32_t inwin[(SegCfg<1>::WIN + 48) / 4];
    CodeTabsT<TabCfg<1>::PBL, uint16_t, 256u> t; /* 256 second-level entries (8-bit link base): 9.4 + 0.5 KB, still 16 wavefronts per CU */
    uint8_t lens[320 + 144];
    uint16_t cl_tab[1 << 7];
    uint32_t cl_len[19];
    uint32_t cl_code[19];
    uint32_t cl_used[19];
#ifdef DEBIG_SCAN_LDS_PAD /* occupancy experiments only */
    uint8_t pad_[DEBIG_SCAN_LDS_PAD];
#endif
};

struct SegTok {
    uint32_t end;        /* lenient end (first symbol start at/after seg_end) */
    uint32_t strict_end; /* where strict decoding stopped */
    uint32_t nbytes, nsym;
    uint32_t flag, status;
    uint32_t ovf; /* a live symbol did not fit the rows left to the stream */
};

#ifdef DEBIG_EMU
DEV_INLINE void st_token(uint32_t *p, uint32_t v) { *p = v; }
#else
DEV_INLINE void st_token(uint32_t *p, uint32_t v) { __builtin_nontemporal_store(v, p); }
#endif

// One symbol with every rare case handled (codes longer than the direct tables, no code at
// all, end of block, symbols 286/287, distance symbols 30/31, the tail gate): the general step
// of the scan, as scan_step_general of inflate_kernel.inc, plus the token.  tok = nullptr:
// positions only.
template <class LDS>
DEV_INLINE void scan_step_general_tok(const LDS &S, uint32_t &lp, uint32_t &live, uint32_t &nbytes, uint32_t &nsym,
                                      uint32_t &flag, uint32_t &status, uint32_t &strict_end, uint32_t &ovf,
                                      int32_t tail_l, uint32_t *tok, uint32_t row_cap)
{
    if (live && (int32_t)lp > tail_l) { flag = FL_TAIL; live = 0; strict_end = lp; }
    Win64 wb = win64(S, lp);
    uint32_t bits = wb.lo;
    uint32_t e = S.t.lit_tab[bits & S.t.mask[CODE_LIT]];
    if (Fmt16::is_link(e) || Fmt16::is_slow(e)) e = huff_slow(bits, S, CODE_LIT, e);
    if (e == 0) { /* no code */
        if (live) { flag = FL_ERR; status = DEBIG_E_NO_CODE; live = 0; strict_end = lp; }
        lp += 1;
        return;
    }
    if (E16_LEN(e) == 0) { /* end of block | symbols 286/287 */
        const uint32_t x = E16_X(e);
        lp += E16_SPECIAL_LEN(e);
        if (live) {
            flag = x == 1u ? (uint32_t)FL_EOB : (uint32_t)FL_ERR;
            status = x == 1u ? 0u : (uint32_t)DEBIG_E_LITLEN_286_287;
            live = 0;
            strict_end = lp;
        }
        return;
    }
    const uint32_t l = E16_LEN(e), nx = E16_X(e), is_len = E16_ISLEN(e);
    const uint32_t vv = E16_V(e) + ((bits >> l) & ((1u << nx) - 1u)); /* the byte | length - 3 */
    uint32_t tokv = vv;
    lp += l + nx;
    if (is_len) {
        uint32_t bits2 = funnel32(wb.hi, wb.lo, l + nx);
        uint32_t de = S.t.dist_tab[bits2 & S.t.mask[CODE_DIST]];
        if (Fmt16::is_link(de) || Fmt16::is_slow(de)) de = huff_slow(bits2, S, CODE_DIST, de);
        if (de == 0 || D16_BAD(de)) { /* no code | distance symbol 30/31 */
            if (live) {
                flag = FL_ERR;
                status = de == 0 ? (uint32_t)DEBIG_E_NO_CODE : (uint32_t)DEBIG_E_DIST_SYMBOL;
                live = 0;
                strict_end = lp;
            }
            lp += de == 0 ? 1u : (de >> 12) & 15u;
            return;
        }
        const uint32_t dx = D16_EXTRA(de), ld = D16_TOTAL(de) - dx;
        const uint32_t dm1 = (D16_M(de) << dx) + ((bits2 >> ld) & ((1u << dx) - 1u));
        lp += ld + dx;
        tokv = TOK_MATCH | (vv << 16) | dm1;
        nbytes += live ? vv + 3u : 0u;
    } else {
        nbytes += live;
    }
    if (live && tok) {
        if (nsym < row_cap) st_token(tok + (size_t)nsym * 64u, tokv);
        else ovf = 1;
    }
    nsym += live;
}

// positions-only round (scan_positions of inflate_kernel.inc on the 16-bit tables): plain short
// symbols in straight-line code, anything else through the general step.  (The lanes must stay
// in step iteration by iteration: a lane that left the loop for a rare symbol and came back
// would run the rest of its segment alone.)
template <class LDS> DEV_INLINE uint32_t scan_positions16(const LDS &S, uint32_t start, uint32_t seg_end, uint32_t &flag)
{
    uint32_t lp = start;
    const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
    uint32_t live = 1, nb = 0, ns = 0, fl = FL_CONT, stt = 0, se = 0, ov = 0; /* only fl is kept: the first terminal event */
    while (lp < seg_end) {
        Win64 wb = win64(S, lp);
        const uint32_t e = S.t.lit_tab[wb.lo & lm];
        const uint32_t l = E16_LEN(e), n1 = l + E16_X(e);
        const uint32_t de = S.t.dist_tab[funnel32(wb.hi, wb.lo, n1) & dm];
        const uint32_t m = E16_LENMASK(e);  /* all ones for a length code */
        const uint32_t y = D16_TOTAL(de) & m; /* bits of the distance part, 0 for a literal */
        // anything but a plain short symbol: a zero length field, or a length code whose distance
        // entry has a zero total.  A lane that guesses decodes garbage, and in garbage these are NOT
        // rare (end of block, symbols 286 / 287, distance symbols 30 / 31: 3-4 % of the symbols of a
        // fixed-Huffman code, so nearly every iteration has a lane on one): the ones that only move
        // the position are handled right here, the general step is for long codes alone
        // (profiles/r03_scan_positions_specials_ab.txt: position rounds 408 k -> 332 k cycles per stream)
        if (umin32(l, y | ~m) == 0) {
            if ((e & 0x1fu) == 0x10u) { lp += E16_SPECIAL_LEN(e); continue; }  /* end of block | 286 / 287 */
            if (e == 0u) { lp += 1u; continue; }                                /* no code starts with these bits */
            if (l != 0u && (de == 0u || (de & 0x8ffu) == 0x800u)) {             /* no distance code | symbol 30 / 31 (not a LINK) */
                lp += n1 + (de == 0u ? 1u : (de >> 12) & 15u);
                continue;
            }
            scan_step_general_tok(S, lp, live, nb, ns, fl, stt, se, ov, 0x7ffffff0, (uint32_t *)nullptr, 0u);
            continue;
        }
        lp += n1 + y;
    }
    flag = fl; /* (terminal events are the full round's business: every lane scans in full after this) */
    return lp;
}

// scan_segment of inflate_kernel.inc (lenient scan, strict view frozen at the first terminal
// event; STOP = strict probe) that also KEEPS what it decodes: the k-th emitting symbol of the
// lane goes to tok[64 k] (tok already points at the lane's column).  Terminal events only happen
// in the general step (end of block and the rest are flagged by a zero length field); the tail
// gate (src/inflate.c:1702) is the loop's bound.
template <bool STOP, class LDS>
DEV_INLINE SegTok scan_segment_tok(const LDS &S, uint32_t start, uint32_t seg_end, int32_t tail_l, uint32_t *tok,
                                   uint32_t row_cap)
{
    uint32_t nbytes = 0, nsym = 0, live = 1, ovf = 0;
    uint32_t lp = start;
    uint32_t flag = FL_CONT, status = 0, strict_end = start;
    const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
    // symbols may start at positions <= tail_l only
    const uint32_t gate_lim = tail_l < 0 ? 0u : (uint32_t)tail_l + 1u;
    const uint32_t lim = gate_lim < seg_end ? gate_lim : seg_end;
    while (lp < lim && (!STOP || live)) {
        Win64 wb = win64(S, lp);
        const uint32_t e = S.t.lit_tab[wb.lo & lm];
        const uint32_t l = E16_LEN(e), nx = E16_X(e);
        const uint32_t n1 = l + nx;
        const uint32_t bits2 = funnel32(wb.hi, wb.lo, n1);
        const uint32_t de = S.t.dist_tab[bits2 & dm];
        const uint32_t m = E16_LENMASK(e);
        const uint32_t dtot = D16_TOTAL(de), y = dtot & m;
        if (umin32(l, y | ~m) == 0) {
            scan_step_general_tok(S, lp, live, nbytes, nsym, flag, status, strict_end, ovf, tail_l, tok, row_cap);
            continue;
        }
        const uint32_t vv = E16_V(e) + ((wb.lo >> l) & ((1u << nx) - 1u));
        const uint32_t dx = D16_EXTRA(de);
        const uint32_t dm1 = (D16_M(de) << dx) + ((bits2 >> (dtot - dx)) & ((1u << dx) - 1u));
        lp += n1 + y;
        // straight-line on purpose (masks instead of ?: keep the compiler from opening an exec region
        // per condition): m is all ones for a length code, live is 0 / 1
        const uint32_t tokv = (vv & ~m) | ((TOK_MATCH | (vv << 16) | dm1) & m);
        const uint32_t can = live & (uint32_t)(nsym < row_cap);
        if (can) st_token(tok + nsym * 64u, tokv);
        ovf |= live ^ can;
        nbytes += (1u + ((vv + 2u) & m)) & (0u - live);
        nsym += live;
    }
    if (live && lp < seg_end && (int32_t)lp > tail_l) { /* the tail gate stopped the lane */
        flag = FL_TAIL;
        live = 0;
        strict_end = lp;
    }
    SegTok r;
    r.flag = flag;
    r.status = status;
    r.strict_end = live ? lp : strict_end;
    r.end = lp;
    r.nbytes = nbytes;
    r.nsym = nsym;
    r.ovf = ovf;
    return r;
}

// BTYPE 1 tables in the scan kernel's format, built once per device (RFC 1951 3.2.6)
__global__ void __launch_bounds__(64) debig_scan_fixed_tables_kernel(uint32_t *out)
{
    __shared__ ScanLds S;
    const uint32_t lane = lane_id();
    for (uint32_t i = lane; i < 288; i += 64)
        S.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    if (lane < 32) S.lens[288 + lane] = 5;
    uint32_t *w = reinterpret_cast<uint32_t *>(&S.t);
    for (uint32_t k = lane; k < sizeof(S.t) / 4; k += 64) w[k] = 0;
    wave_local_sync();
    build_code(S, CODE_LIT, S.lens, 288);
    build_code(S, CODE_DIST, S.lens + 288, 32);
    wave_local_sync();
    for (uint32_t k = lane; k < sizeof(S.t) / 4; k += 64) out[k] = w[k];
}

#ifdef DEBIG_PROFILE /* the phase counters need registers: diagnostic builds run 3 waves per SIMD */
#define DEBIG_SCAN_WAVES_PER_EU 3
#define DEBIG_LZ_WAVES_PER_EU 2
#endif
// Speculation schedule of a symbol window, measured on the emulator (rounds per window, 64 KiB
// streams: fixed-Huffman text / dynamic text / image rows) and on the GPU:
//   2 position rounds (fixed), 1 (dynamic), no lead   3.07 / 3.24 / 2.61  (the one-kernel path's schedule)
//   1 position round, lead 272 bits                    2.26 / 2.62 / 2.22  (round 0 costs 1.5 segments)
#ifndef DEBIG_SCAN_LEAD_BITS
#define DEBIG_SCAN_LEAD_BITS 272u
#endif
#ifndef DEBIG_SCAN_POS_ROUNDS
#define DEBIG_SCAN_POS_ROUNDS 1u
#endif
#ifndef DEBIG_SCAN_WAVES_PER_EU
#define DEBIG_SCAN_WAVES_PER_EU 4
#endif
#ifndef DEBIG_LZ_WAVES_PER_EU
#define DEBIG_LZ_WAVES_PER_EU 4
#endif
#ifdef DEBIG_EMU
#define DEBIG_SCAN_ATTRS
#define DEBIG_LZ_ATTRS
#else
#define DEBIG_SCAN_ATTRS __attribute__((amdgpu_waves_per_eu(DEBIG_SCAN_WAVES_PER_EU)))
#define DEBIG_LZ_ATTRS __attribute__((amdgpu_waves_per_eu(DEBIG_LZ_WAVES_PER_EU)))
#endif

// The scan of one stream (CHUNKED = false: slot index = stream index) or of one chunk of a large
// stream (CHUNKED = true, inflate_chunk_kernel.inc: from the block header at start_bit to the
// first block boundary at or beyond stop_bit; nothing is written to the recipient, stored blocks
// become records, the aliasing replay is recorded for every block of the last chunk).
template <bool CHUNKED>
DEV_INLINE void scan_body(ScanLds &S, const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                          const debig_stream &st, const uint32_t sid /* slot index */,
                          const uint32_t *__restrict__ fixed_tabs, debig_ws_slot *__restrict__ slots,
                          debig_ws_rec *__restrict__ recs, uint32_t *__restrict__ rows, debig_result *results,
                          const uint64_t start_bit, const uint64_t stop_bit, const int last_chunk,
                          uint32_t *state_out = nullptr /* what slots[sid].state becomes (wave-uniform) */)
{
    if (state_out) *state_out = DEBIG_E_RETRY;
    PROF_DECL
    const uint32_t lane = lane_id();
    const debig_ws_slot slot = slots[sid];
    const uint8_t *in = in_arena + st.in_off;
    const uint64_t in_len = st.in_len;
    uint8_t *out = out_arena + st.out_off;
    debig_ws_rec *myrec = recs + slot.rec0;
    uint32_t *myrows = rows + slot.row0 * 64u;

    uint32_t status = DEBIG_OK, final_set = 0;
    uint32_t n_blocks = 0, n_windows = 0, n_rounds = 0;
    int64_t end_bits = 0;
    int tables = 0;
    int64_t staged_base = 0;
    int staged_valid = 0;
    int short_mode = 0;
    uint64_t outpos = 0;     /* bytes the stream has produced so far (if no match fails in the LZ77 kernel) */
    uint32_t row_cur = 0;    /* rows used */
    uint32_t rec_cur = 0;    /* records used; the last one is kept for REC_END */
    const uint32_t rec_lim = slot.recs ? slot.recs - 1u : 0u;

#define SCAN_EMIT(KIND, ROW, A, B, C, D)                                                        \
    do {                                                                                         \
        if (rec_cur >= rec_lim) { status = DEBIG_E_RETRY; }                                      \
        else {                                                                                   \
            if (lane == 0) {                                                                     \
                debig_ws_rec rr;                                                                 \
                rr.kind = (KIND); rr.row = (ROW); rr.a = (A); rr.b = (B); rr.c = (C); rr.d = (D); \
                myrec[rec_cur] = rr;                                                             \
            }                                                                                    \
            rec_cur++;                                                                           \
        }                                                                                        \
    } while (0)

    if (slot.recs == 0) return; /* no room even for the verdict: state stays RETRY */
    if (!CHUNKED && !(st.flags & DEBIG_STREAM_NO_REF_GATES)) { /* chunked: the chain kernel applies the gates */
        if (st.out_cap < in_len) status = DEBIG_E_GATE_RECIPIENT_SMALL;
        else if (in_len < 5) status = DEBIG_E_GATE_INPUT_SHORT;
    }
    uint32_t chunk_flags = 0;
    if (status == DEBIG_OK) {
        final_set = 1;
        int64_t bitpos = CHUNKED ? (int64_t)start_bit : 0;
        int more = 1;
        while (more && status == DEBIG_OK) {
            if (CHUNKED && (uint64_t)bitpos >= stop_bit) { /* a block boundary at or beyond the next chunk's start */
                if ((uint64_t)bitpos == stop_bit) chunk_flags |= SLOT_MATCHED;
                break;
            }
            // ---- block header (as debig_inflate_kernel)
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
                if (!CHUNKED && outpos + len > st.out_cap) { status = DEBIG_E_OUTPUT_FULL; break; }
                SCAN_EMIT(REC_STORED, 0u, (uint32_t)CHUNKED, 0u, (uint64_t)len, (uint64_t)(hb.pos >> 3));
                if (status != DEBIG_OK) break;
                if (!CHUNKED) stored_copy<1>(in, in_len, hb.pos >> 3, out + outpos, len); /* chunked: the LZ77 kernel copies */
                outpos += len;
                bitpos = hb.pos + 8 * (int64_t)len;
                continue;
            }
            int fixed = (btype == 1);
            // chunked: the output position is not known here; every block of the LAST chunk records its
            // table image and the LZ77 kernel applies the condition
            int need_p2 = CHUNKED ? (st.p2_on && last_chunk) : (st.p2_on && ((int64_t)outpos > st.p2_s0));
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
                // the table image the reference writes over [p2_s0, outpos): applied by the LZ77
                // kernel at this point of the stream (it owns the output); the code-length table
                // of a dynamic block travels in one token row
                if (row_cur >= slot.rows) { status = DEBIG_E_RETRY; break; }
                if (!fixed && lane < 19) {
                    uint32_t *rw = myrows + (size_t)row_cur * 64u;
                    rw[3 * lane] = S.cl_code[lane];
                    rw[3 * lane + 1] = S.cl_used[lane];
                    rw[3 * lane + 2] = S.cl_len[lane];
                }
                SCAN_EMIT(REC_P2, row_cur, (uint32_t)fixed, 0u, outpos, 0ull);
                if (status != DEBIG_OK) break;
                row_cur++;
            }
            bitpos = hb.pos;
            PROF_END(3);

            // ---- symbol windows
            int block_done = 0;
            while (!block_done && status == DEBIG_OK) {
                n_windows++;
                if (row_cur + 2u > slot.rows) { status = DEBIG_E_RETRY; break; }
                const uint32_t row_cap = slot.rows - row_cur - 1u; /* token rows left behind the counts row */
                uint32_t *tok = myrows + (size_t)(row_cur + 1u) * 64u + lane;
                SegTok si;
                si.end = 0; si.strict_end = 0; si.nbytes = 0; si.nsym = 0; si.flag = FL_CONT; si.status = 0; si.ovf = 0;
                uint32_t start = 0, first_term = 64;
                int probe_hit = 0;
                if (short_mode) {
                    wbase = stage_window_cached(S, in, in_len, bitpos >> 3, DEBIG_PROBE_NEED, 0, staged_base, staged_valid);
                    org = 8 * wbase;
                    int64_t ptl = 8 * ((int64_t)in_len - 1) - org;
                    const int32_t ptail = ptl < -1 ? -1 : (ptl > 0x7ffffff0 ? 0x7ffffff0 : (int32_t)ptl);
                    start = (uint32_t)(bitpos - org);
                    if (lane == 0) si = scan_segment_tok<true>(S, start, start + SEG_BITS, ptail, tok, row_cap);
                    n_rounds++;
                    probe_hit = wave_bcast_u32(si.flag, 0) != FL_CONT;
                    if (probe_hit) first_term = 0;
                    else {
                        short_mode = 0;
                        si.end = 0; si.strict_end = 0; si.nbytes = 0; si.nsym = 0; si.flag = FL_CONT; si.status = 0; si.ovf = 0;
                    }
                }
                if (!probe_hit) {
                    PROF_BEGIN();
                    wbase = stage_window_cached(S, in, in_len, bitpos >> 3, WIN_BYTES + 16u, 1, staged_base, staged_valid);
                    PROF_END(0);
                    org = 8 * wbase;
                    const uint32_t seg_lo = lane * SEG_BITS;
                    const uint32_t seg_end = seg_lo + SEG_BITS;
                    // round 0 starts from a guess DEBIG_SCAN_LEAD_BITS before the segment: the lane
                    // arrives at its own segment already in step with the real symbol sequence
                    start = (lane == 0) ? (uint32_t)(bitpos - org) : seg_lo - DEBIG_SCAN_LEAD_BITS;
                    int64_t tl = 8 * ((int64_t)in_len - 1) - org;
                    const int32_t tail_l = tl < -1 ? -1 : (tl > 0x7ffffff0 ? 0x7ffffff0 : (int32_t)tl);
                    int dirty = 1;
                    si.end = start; si.strict_end = start;
                    first_term = 64;
                    // DEBIG_SCAN_POS_ROUNDS rounds only chase positions (cheap); then every lane scans
                    // in full once (counts, the strict view, tokens), then only lanes whose start moved
                    const uint32_t npos = DEBIG_SCAN_POS_ROUNDS;
                    for (uint32_t round = 0; round < 70u + npos; round++) {
                        PROF_BEGIN();
                        if (round < npos) { if (dirty) si.end = scan_positions16(S, start, seg_end, si.flag); }
                        else if (dirty) si = scan_segment_tok<false>(S, start, seg_end, tail_l, tok, row_cap);
                        if (round < npos) { PROF_END(1); } else { PROF_END(2); }
                        dirty = round == npos - 1u;
                        n_rounds++;
                        uint32_t prev_end = __shfl_up(si.end, 1);
                        unsigned long long cont = __ballot(si.flag == FL_CONT);
                        first_term = (~cont == 0ull) ? 64u : (uint32_t)(__ffsll(~cont) - 1);
                        if (lane > 0 && start != prev_end) {
                            start = prev_end;
                            dirty = 1;
                        }
                        if (round >= npos && !__any(dirty && lane <= first_term)) break;
                    }
                    short_mode = first_term == 0;
                }
                PROF_BEGIN();
                const uint32_t last = first_term < 64u ? first_term : 63u;
                const int used = lane <= last;
                const uint32_t wflag = wave_bcast_u32(si.flag, last);
                const uint32_t wstatus = wave_bcast_u32(si.status, last);
                const int64_t wend = org + (int64_t)wave_bcast_u32(si.strict_end, last);
                if (__any(used && si.ovf)) { status = DEBIG_E_RETRY; break; }
                const uint32_t nbytes = used ? si.nbytes : 0u;
                const uint32_t nsym = used ? si.nsym : 0u;
                uint32_t wtotal;
                (void)wave_excl_scan_u32(nbytes, &wtotal);
                const uint32_t max_sym = wave_max_u32(nsym);
                myrows[(size_t)row_cur * 64u + lane] = nsym | (nbytes << 10);
                SCAN_EMIT(REC_WIN, row_cur, (last + 1u) | (wflag << 8), wstatus, (uint64_t)wtotal, 0ull);
                if (status != DEBIG_OK) break;
                row_cur += 1u + max_sym;
                outpos += wtotal;
                bitpos = wend;
                PROF_END(4);
                if (wflag == FL_EOB) block_done = 1;
                else if (wflag == FL_TAIL) { block_done = 1; more = 0; }
                else if (wflag == FL_ERR) { status = wstatus; }
            }
        }
        end_bits = bitpos;
        if (CHUNKED && !more && status == DEBIG_OK) chunk_flags |= SLOT_FINAL | (last_chunk ? SLOT_MATCHED : 0u);
    }
#undef SCAN_EMIT
    if (state_out) *state_out = (status == DEBIG_E_RETRY || (CHUNKED && status != DEBIG_OK)) ? (uint32_t)DEBIG_E_RETRY : (uint32_t)DEBIG_OK;
    if (lane == 0) {
        debig_ws_rec rr;
        rr.kind = REC_END;
        rr.row = final_set;
        rr.a = status;
        rr.b = n_blocks;
        rr.c = (uint64_t)end_bits;
        rr.d = (uint64_t)n_windows | ((uint64_t)n_rounds << 32);
        myrec[rec_cur < slot.recs ? rec_cur : slot.recs - 1u] = rr;
        // chunked: any failure of a chunk (a real one or a chunk that started on a false block
        // header) sends the stream to the one-kernel path, which owns the exact error semantics
        slots[sid].state = (status == DEBIG_E_RETRY || (CHUNKED && status != DEBIG_OK)) ? (uint32_t)DEBIG_E_RETRY : (uint32_t)DEBIG_OK;
        if (CHUNKED) {
            slots[sid].flags = chunk_flags;
            slots[sid].out_total = outpos;
            slots[sid].end_bit = (uint64_t)end_bits;
            slots[sid].n_blocks = n_blocks; slots[sid].n_windows = n_windows; slots[sid].n_rounds = n_rounds;
        }
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
        /* diagnostic builds: the scan kernel's phase cycles travel in the result (kept by the LZ77
         * kernel): 0 stage, 1 position rounds, 2 full rounds, 3 header+tables, 4 window records, 6 total */
        if (!CHUNKED) PROF_STORE(results[sid]);
#endif
    }
    (void)results;
}

// ------------------------------------------------------------------ LZ77 half
#ifndef DEBIG_PROFILE_LZ
#define DEBIG_PROFILE_LZ 0
#endif
#ifndef DEBIG_T2
#define DEBIG_T2 5120 /* output tile of the LZ77 kernel: 32 segments of 68 bytes at ratio 2 fit in one piece */
#endif
#define LZ_MAP_WORDS (((DEBIG_T2 + DEBIG_TSLACK + 2047) / 2048) * 64 + 16)
// E_ = uint16_t (chunk path): WIDE elements -- an output "byte" is the pair {a, b} of what it would
// be behind two synthetic histories (inflate_chunk_kernel.inc: a == b is a literal, a != b names one
// history byte), replayed as ONE element: every position, length, distance, bitmap and list below
// counts ELEMENTS, only the accesses to the tile and to the output plane know the element's size.
// (Round 2 replayed two byte planes side by side: every copy twice, two gather lines per far match.)
template <int T2_ = DEBIG_T2, class E_ = uint8_t> struct __attribute__((aligned(16))) LzLdsT {
    static constexpr int NW = 1;
    typedef E_ Elem;
    static constexpr int ES = (int)sizeof(E_);
    static constexpr int T2 = T2_; /* tile elements */
    static constexpr uint32_t MAP_WORDS = (((uint32_t)T2_ + DEBIG_TSLACK + 2047u) / 2048u) * 64u + 16u; /* a bit per element */
    E_ tile[T2_ + DEBIG_TSLACK];
    uint32_t bitmap[MAP_WORDS]; /* whole 2048-byte spans: the span loops read 64 words each */
    uint32_t farmap[MAP_WORDS];
    uint32_t pend[MAP_WORDS];
    uint16_t mpos[1][MPOS_CAP];
    uint32_t internal_err;
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
    uint64_t nprof[4]; /* diagnostic builds: near_groups_r's cycles: group set-up | dependency search | rounds | one-at-a-time copies */
#endif
#ifdef DEBIG_LZ_LDS_PAD /* occupancy experiments only */
    uint8_t pad_[DEBIG_LZ_LDS_PAD];
#endif
};
typedef LzLdsT<> LzLds;
// A larger tile for the kernels that run few wavefronts per CU anyway (the strand pipeline up to 1280 streams, the fused
// PNG kernel up to 512 images): every tile costs a flush, a wait for it, a far and a near pass whatever it holds, and data
// that turns 30 KB into 4 MB fills a 5 KB tile with two or three token units.  Measured with the tile of every kernel
// changed (profiles/r04_lz_tile_ab.txt): 128 flat-colour PNG streams 15.0 -> 10.8 ms, 512 x 1 MiB text 132 -> 148 GB/s,
// 256 x 1 MiB 70 -> 78.5; chunk tasks and the 16-wavefronts-per-CU kernels lose occupancy to it and keep theirs.
#ifndef DEBIG_T2_BIG
#define DEBIG_T2_BIG 12288
#endif
typedef LzLdsT<DEBIG_T2_BIG> LzLdsBig;
// a wide tile seen as bytes by the helpers written for bytes (flush_range)
struct LzByteView {
    static constexpr int NW = 1;
    uint8_t *tile;
};
// tile_base for output position pos: (out + ES * tile_base) % 16 == 0 (the plane is 2-byte aligned)
template <class LDS> DEV_INLINE int64_t lz_anchor(const uint8_t *out, int64_t pos)
{
    if (LDS::ES == 1) return align_anchor(out, pos);
    const uintptr_t a = (uintptr_t)out + 2u * (uintptr_t)pos;
    return pos - (int64_t)((a & 15u) >> 1);
}
// fence = 0: the stores stay in flight; the caller fences before the output is read or written again
template <class LDS> DEV_INLINE void lz_flush_range(LDS &S, OutState &O, int64_t from, int64_t to, int fence = 1)
{
    if constexpr (LDS::ES == 2) {
        LzByteView V;
        V.tile = reinterpret_cast<uint8_t *>(S.tile);
        OutState OB = O;
        OB.tile_base = 2 * O.tile_base;
        flush_range(V, OB, 2 * from, 2 * to, fence);
    } else {
        flush_range(S, O, from, to, fence);
    }
}
// the bytes below O.lds_from are in L2 (the caller has waited for its stores): say so to whoever reads the recipient
// behind this wavefront (debig_png_fused_kernel; a null pointer everywhere else)
DEV_INLINE void lz_publish(const OutState &O)
{
    if (O.pub) {
        int64_t v = O.lds_from < O.pub_cap ? O.lds_from : O.pub_cap;
        if (v > 0xffffff00ll) v = 0xffffff00ll;
        if (lane_id() == 0) *O.pub = v < 0 ? 0u : (uint32_t)v;
    }
}
template <class LDS> DEV_INLINE void lz_flush_all(LDS &S, OutState &O, int fence = 1)
{
    lz_flush_range(S, O, O.lds_from, O.outpos, fence);
    O.lds_from = O.outpos;
    O.tile_base = lz_anchor<LDS>(O.out, O.outpos);
    if (fence) lz_publish(O);
}
// one element of the output at position p < the write position, from the tile or from the plane
#ifdef DEBIG_EMU
static inline uint16_t ld_hist_u16(const uint16_t *p) { return *p; }
#else
DEV_INLINE uint16_t ld_hist_u16(const uint16_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif
template <class LDS> DEV_INLINE typename LDS::Elem lz_ld_plane(const OutState &O, int64_t p)
{
    if constexpr (LDS::ES == 2) return ld_hist_u16(reinterpret_cast<const uint16_t *>(O.out) + p);
    else return ld_hist_u8(O.out + p);
}
template <class LDS> DEV_INLINE typename LDS::Elem lz_hist_elem(const LDS &S, const OutState &O, int64_t p)
{
    if (p >= O.lds_from) return S.tile[p - O.tile_base];
    return lz_ld_plane<LDS>(O, p);
}
// copy_match_wave of inflate_kernel.inc on elements
template <class LDS> DEV_INLINE void lz_copy_match_wave(LDS &S, const OutState &O, uint32_t lp, uint32_t ll, uint32_t ld)
{
    if constexpr (LDS::ES == 1) {
        copy_match_wave(S, O, lp, ll, ld);
    } else {
        const uint32_t lane = lane_id();
        const int64_t ls = O.tile_base + (int64_t)lp - (int64_t)ld;
        const int overlap = ld < ll;
        const uint32_t M = overlap ? ((1u << 20) + ld - 1u) / ld : 0u;
        const int in_tile = ls >= O.lds_from;
        const uint32_t sr = (uint32_t)(ls - O.tile_base);
        typename LDS::Elem tmp[5];
        DEV_UNROLL
        for (uint32_t it = 0; it < 5; it++) {
            const uint32_t k = it * 64u + lane;
            if (k < ll) {
                const uint32_t kk = overlap ? k - ((k * M) >> 20) * ld : k;
                tmp[it] = in_tile ? S.tile[sr + kk] : lz_hist_elem(S, O, ls + kk);
            }
        }
        DEV_UNROLL
        for (uint32_t it = 0; it < 5; it++) {
            const uint32_t k = it * 64u + lane;
            if (k < ll) S.tile[lp + k] = tmp[it];
        }
    }
}

#ifdef DEBIG_EMU
DEV_INLINE uint32_t ld_token(const uint32_t *p) { return *p; }
#else
DEV_INLINE uint32_t ld_token(const uint32_t *p) { return __builtin_nontemporal_load(p); }
#endif
// ---- match copies with unaligned accesses.  gfx950 runs in unaligned access mode (hipcc itself
// emits unaligned ds_write_b64 / global_load_dword for packed structs), so a 3..16 byte match is
// ONE 16-byte load and at most TWO stores: the first 8 (4, 2) bytes and the last 8 (4, 1) bytes of
// the match, overlapping in the middle.  (inflate_kernel.inc's versions, written for aligned
// dwords, take 5 loads and up to 16 byte stores.)
struct __attribute__((packed)) pk_u16 { uint16_t v; };
struct __attribute__((packed)) pk_u32 { uint32_t v; };
struct __attribute__((packed)) pk_u64 { uint64_t v; };
struct __attribute__((packed)) pk_u128 { uint32_t x, y, z, w; };
// 16 history bytes at any recipient position, served by L2 (never a possibly stale L1 line) and
// KEPT there: sc1 buffer loads.  (Round 2 used non-temporal loads: the hint marks the lines as
// streaming, L2 and the Infinity Cache drop them first, and nearly every far match went to HBM as
// a random 64-byte read -- measured on 4096 x 64 KiB fixed-Huffman streams, profiles/r03_hist_policy.txt:
// LZ77 kernel 586 us with nt, 420 us with sc1.)  The buffer descriptor spans the recipient from
// 32 KiB before the tile: offsets fit 32 bits whatever the recipient's size, and the range check
// of the descriptor never lets a load touch bytes beyond recipient_size.
#ifdef DEBIG_EMU
struct HistBuf { const uint8_t *out; };
DEV_INLINE HistBuf hist_buf(const uint8_t *out, uint64_t, int64_t, int64_t = 32768) { HistBuf h; h.out = out; return h; }
DEV_INLINE void ld_hist_16(const HistBuf &h, int64_t src, uint32_t &x, uint32_t &y, uint32_t &z, uint32_t &w)
{
    pk_u128 v;
    memcpy(&v, h.out + src, 16);
    x = v.x; y = v.y; z = v.z; w = v.w;
}
#else
struct HistBuf {
    __amdgpu_buffer_rsrc_t rs;
    int64_t org; /* recipient position of the descriptor's byte 0 (> -16) */
};
DEV_INLINE HistBuf hist_buf(const uint8_t *out, uint64_t out_cap, int64_t tile_base, int64_t back = 32768)
{
    const int64_t hb = tile_base > back ? tile_base - back : 0;
    const uintptr_t a = ((uintptr_t)out + (uintptr_t)hb) & ~(uintptr_t)15;
    HistBuf h;
    h.org = (int64_t)a - (int64_t)(uintptr_t)out;
    const int64_t left = (int64_t)out_cap - h.org;
    h.rs = __builtin_amdgcn_make_buffer_rsrc((void *)a, 0, left > 0x7fffffff ? 0x7fffffff : (int)left, 0x00020000);
    return h;
}
DEV_INLINE void ld_hist_16(const HistBuf &h, int64_t src, uint32_t &x, uint32_t &y, uint32_t &z, uint32_t &w)
{
    typedef unsigned int u32x4v __attribute__((__vector_size__(16)));
#if defined(DEBIG_ABLATE) && (DEBIG_ABLATE & 4) /* timing experiment: no gather traffic (wrong output) */
    u32x4v q = {(unsigned)src, (unsigned)src, (unsigned)src, (unsigned)src};
#else
    const u32x4v q = __builtin_amdgcn_raw_buffer_load_b128(h.rs, (int)(src - h.org), 0, 16 /* sc1 */);
#endif
    x = q[0]; y = q[1]; z = q[2]; w = q[3];
}
#endif
// store the first `len` (3..16) bytes of {x, y, z, w} at tile + p
template <class LDS>
DEV_INLINE void st_match_bytes(LDS &S, uint32_t p, uint32_t len, uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    uint8_t *d = S.tile + p;
    if (len >= 8u) {
        reinterpret_cast<pk_u64 *>(d)->v = ((uint64_t)y << 32) | x;
        // bytes [len - 8, len): a 64-bit window of the 128 bits at byte offset 0..8
        const uint32_t o = len - 8u;
        const uint32_t a0 = o < 4u ? x : y, a1 = o < 4u ? y : z, a2 = o < 4u ? z : w;
        const uint32_t lo = alignbyte32(a1, a0, o & 3u), hi = alignbyte32(a2, a1, o & 3u);
        const uint32_t lo8 = o == 8u ? z : lo, hi8 = o == 8u ? w : hi;
        reinterpret_cast<pk_u64 *>(d + o)->v = ((uint64_t)hi8 << 32) | lo8;
    } else if (len >= 4u) {
        reinterpret_cast<pk_u32 *>(d)->v = x;
        const uint32_t o = len - 4u; /* 0..3 */
        reinterpret_cast<pk_u32 *>(d + o)->v = alignbyte32(y, x, o);
    } else {
        reinterpret_cast<pk_u16 *>(d)->v = (uint16_t)x;
        d[2] = (uint8_t)(x >> 16);
    }
}

// wide elements: store `len` (3..16) elements at tile + p; A = source elements [0, 8), B = source
// elements [len - 8, len) (read only for len > 8): the two halves overlap in the middle, nothing is
// shuffled through registers
template <class LDS>
DEV_INLINE void st_match_wide(LDS &S, uint32_t p, uint32_t len, const uint32_t A[4], const uint32_t B[4])
{
    uint16_t *d = reinterpret_cast<uint16_t *>(S.tile) + p;
    if (len >= 8u) {
        reinterpret_cast<pk_u64 *>(d)[0].v = ((uint64_t)A[1] << 32) | A[0];
        reinterpret_cast<pk_u64 *>(d)[1].v = ((uint64_t)A[3] << 32) | A[2];
        if (len > 8u) {
            pk_u64 *e = reinterpret_cast<pk_u64 *>(d + (len - 8u));
            e[0].v = ((uint64_t)B[1] << 32) | B[0];
            e[1].v = ((uint64_t)B[3] << 32) | B[2];
        }
    } else if (len >= 4u) {
        reinterpret_cast<pk_u64 *>(d)->v = ((uint64_t)A[1] << 32) | A[0];
        const uint32_t o = len - 4u; /* elements [o, o + 4) of A, o = 0..3 */
        const uint32_t a0 = o < 2u ? A[0] : A[1], a1 = o < 2u ? A[1] : A[2], a2 = o < 2u ? A[2] : A[3];
        const uint32_t sh = (o & 1u) * 2u;
        const uint32_t lo = alignbyte32(a1, a0, sh), hi = alignbyte32(a2, a1, sh);
        reinterpret_cast<pk_u64 *>(d + o)->v = ((uint64_t)hi << 32) | lo;
    } else {
        reinterpret_cast<pk_u32 *>(d)->v = A[0];
        d[2] = (uint16_t)A[1];
    }
}

// copy the far matches listed in S.mpos[0][0..total): DEPTH groups of 64 in flight (the source
// reads are random 16-byte gathers from L2 / Infinity Cache: latency is hidden by issuing them all)
template <int DEPTH, class LDS> DEV_INLINE void far_groups(LDS &S, OutState &O, uint32_t total)
{
    const uint32_t lane = lane_id();
    constexpr int ES = LDS::ES;
    const HistBuf HA = hist_buf(O.out, (uint64_t)ES * O.out_cap, (int64_t)ES * O.tile_base, 32768 * ES);
    for (uint32_t g0 = 0; g0 < total; g0 += 64u * DEPTH) {
        uint32_t mp[DEPTH], mlen[DEPTH];
        uint32_t t[DEPTH][4];
        uint32_t tb[DEPTH][4]; /* wide elements: the last 8 elements of a match longer than 8 */
        int64_t msrc[DEPTH];
        int quick[DEPTH]; /* one 16-byte read + two stores */
        DEV_UNROLL
        for (int d = 0; d < DEPTH; d++) {
            uint32_t q = g0 + (uint32_t)d * 64u + lane;
            mp[d] = 0; mlen[d] = 0; msrc[d] = 0; quick[d] = 0;
            if (q < total) {
                uint32_t p = S.mpos[0][q];
                uint32_t len = (uint32_t)S.tile[p] + 3u;
                uint32_t dist = ((uint32_t)S.tile[p + 1] | ((uint32_t)S.tile[p + 2] << 8)) + 1u;
                mp[d] = p;
                msrc[d] = O.tile_base + (int64_t)p - (int64_t)dist;
                mlen[d] = len;
                // a whole 16-byte read must stay inside the recipient
                quick[d] = len <= 16u && (uint64_t)(msrc[d] + 16) <= O.out_cap;
                if (quick[d]) ld_hist_16(HA, (int64_t)ES * msrc[d], t[d][0], t[d][1], t[d][2], t[d][3]);
                if (ES == 2 && quick[d] && len > 8u)
                    ld_hist_16(HA, 2 * (msrc[d] + (int64_t)len - 8), tb[d][0], tb[d][1], tb[d][2], tb[d][3]);
            }
        }
        DEV_UNROLL
        for (int d = 0; d < DEPTH; d++) {
            if constexpr (ES == 2) {
                if (quick[d]) st_match_wide(S, mp[d], mlen[d], t[d], tb[d]);
            } else {
                if (quick[d]) st_match_bytes(S, mp[d], mlen[d], t[d][0], t[d][1], t[d][2], t[d][3]);
            }
        }
        // long far matches (and the rare ones at the very end of the recipient): one at a
        // time, all 64 lanes copy
        DEV_UNROLL
        for (int d = 0; d < DEPTH; d++) {
            unsigned long long lm = __ballot(mlen[d] != 0 && !quick[d]);
            while (lm) {
                int sl = __ffsll(lm) - 1;
                lm &= lm - 1;
                uint32_t lp = __shfl(mp[d], sl);
                uint32_t ll = __shfl(mlen[d], sl);
                int64_t ls = __shfl(msrc[d], sl);
                typename LDS::Elem tmp[5];
                DEV_UNROLL
                for (uint32_t it = 0; it < 5; it++) {
                    uint32_t k = it * 64u + lane;
                    if (k < ll) tmp[it] = lz_ld_plane<LDS>(O, ls + k);
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

#ifndef LZ_SPAN_FAR_DEPTH
#define LZ_SPAN_FAR_DEPTH 2 /* groups of 64 far matches in flight, span-wise copy */
#endif
// far_copy of inflate_kernel.inc with the copies above.  recip_end = recipient_size: a 16-byte
// read that would pass it goes byte by byte (nothing beyond the recipient is ever touched).
template <class LDS> DEV_INLINE void far_copy_u(LDS &S, OutState &O, uint32_t from_rel, uint32_t to_rel)
{
    const uint32_t lane = lane_id();
    wave_local_sync();
    for (uint32_t span = (from_rel >> 11); span < ((to_rel + 2047u) >> 11); span++) {
        uint32_t wbase = span * 64u + lane;
        uint32_t w = S.farmap[wbase];
        uint32_t p0 = wbase * 32u;
        if (p0 + 32u <= from_rel || p0 >= to_rel) w = 0;
        else {
            if (p0 < from_rel) w &= ~0u << (from_rel - p0);
            if (p0 + 32u > to_rel) w &= (1u << (to_rel - p0)) - 1u;
        }
        S.farmap[wbase] = 0;
        if (!__any(w != 0)) continue; /* no far match starts in this span */
        uint32_t total;
        uint32_t pre = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        {
            uint32_t k = pre, ww = w;
            while (ww) {
                uint32_t bit = (uint32_t)__ffs(ww) - 1u;
                ww &= ww - 1u;
                S.mpos[0][k++] = (uint16_t)(p0 + bit);
            }
        }
        wave_local_sync();
        far_groups<LZ_SPAN_FAR_DEPTH>(S, O, total);
        wave_local_sync(); /* S.mpos is rewritten by the next span */
    }
    wave_local_sync();
}

// copy_short_match of inflate_kernel.inc (3..16 bytes, non-overlapping, source in the LDS tile)
// with two unaligned 8-byte reads and st_match_bytes
template <class LDS> DEV_INLINE void copy_short_match_u(LDS &S, int mine, uint32_t p, uint32_t len, uint32_t sr)
{
    if (mine) {
        const pk_u64 *sp = reinterpret_cast<const pk_u64 *>(S.tile + sr);
        const uint64_t lo = sp[0].v, hi = sp[1].v;
        if constexpr (LDS::ES == 2) {
            const uint32_t A[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
            uint32_t B[4] = {0, 0, 0, 0};
            if (len > 8u) {
                const pk_u64 *sq = reinterpret_cast<const pk_u64 *>(S.tile + sr + (len - 8u));
                const uint64_t l2 = sq[0].v, h2 = sq[1].v;
                B[0] = (uint32_t)l2; B[1] = (uint32_t)(l2 >> 32); B[2] = (uint32_t)h2; B[3] = (uint32_t)(h2 >> 32);
            }
            st_match_wide(S, p, len, A, B);
        } else {
            st_match_bytes(S, p, len, (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        }
    }
}

// resolve_matches_groups of inflate_kernel.inc with copy_short_match_u, and the dependencies of a group kept in
// REGISTERS instead of the pending bitmap (round 4).  A group is 64 consecutive near matches
// in position order, and every group before it is finished when it starts: the only bytes of a match's source that can
// still be pending are destinations of matches of the SAME group, i.e. of lanes below it -- and, positions being
// sorted and destinations disjoint, of a contiguous range of lanes [lo, hi), found by two binary searches over the
// lanes' start / end positions (six shuffle steps, both searches side by side).  A match is ready when none of those
// lanes is pending: a ballot and two ANDs per round, against two pending-bitmap reads, one or two LDS atomics and two
// waits per round and lane with the bitmap -- whose rounds were a chain of four dependent LDS round trips
// (pending bits -> source -> destination -> pending bits).  Here a round is source -> destination, and the next
// round's reads may follow the writes at once (one wavefront: the LDS executes its instructions in order).
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
#define NPROF_T() __builtin_amdgcn_s_memtime()
#define NPROF_ADD(i, t0) do { if (lane_id() == 0) S.nprof[i] += __builtin_amdgcn_s_memtime() - (t0); } while (0)
#else
#define NPROF_T() 0ull
#define NPROF_ADD(i, t0) do { (void)(t0); } while (0)
#endif
template <class LDS> DEV_INLINE void near_groups_r(LDS &S, OutState &O, uint32_t total)
{
    static_assert(LDS::NW == 1, "one wavefront per tile");
    const uint32_t lane = lane_id();
    const int64_t lds_rel0 = O.lds_from - O.tile_base; /* tile bytes below this are not in LDS */
    for (uint32_t g = 0; g < total; g += 64) {
        const uint32_t q = g + lane;
        int pending = q < total;
        uint32_t p = 0xffffffffu, len = 0, dist = 1;
        const uint64_t nt0 = NPROF_T();
        if (pending) {
            p = S.mpos[0][q];
            len = (uint32_t)S.tile[p] + 3u;
            dist = ((uint32_t)S.tile[p + 1] | ((uint32_t)S.tile[p + 2] << 8)) + 1u;
        }
        const uint32_t pe = pending ? p + len : 0xffffffffu; /* end of my destination; ascending with the lane, like p */
        const int64_t src_rel = (int64_t)p - (int64_t)dist;   /* tile relative, may be < 0 */
        const uint32_t span_len = len < dist ? len : dist;     /* distinct source bytes   */
        int64_t t0 = src_rel > lds_rel0 ? src_rel : lds_rel0;  /* the part of the source that lives in the tile */
        int64_t t1 = src_rel + (int64_t)span_len;
        const int has_src = pending && t0 < t1;
        const uint32_t u0 = has_src ? (uint32_t)t0 : 0u, u1 = has_src ? (uint32_t)t1 : 0u;
        const int src_in_lds = src_rel >= lds_rel0;
        NPROF_ADD(0, nt0);
        const uint64_t nt1 = NPROF_T();
        // lanes whose destination meets [u0, u1): lo = lanes that end at or below u0, hi = lanes that start below u1
        uint32_t lo = 0, hi = 0;
        uint64_t need = 0;
        // (text: most near matches copy from literals or from matches of earlier groups -- no source reaches past the group's
        // first destination, and there is nothing to search for)
        const uint32_t p_first = wave_bcast_u32(p, 0);
        if (__any(has_src && u1 > p_first)) {
DEV_UNROLL
            for (uint32_t step = 32; step; step >>= 1) {
                const uint32_t el = (uint32_t)__shfl((int)pe, (int)(lo + step - 1u));
                const uint32_t pl = (uint32_t)__shfl((int)p, (int)(hi + step - 1u));
                if (el <= u0) lo += step;
                if (pl < u1) hi += step;
            }
            if (has_src && hi > lo) need = ((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull); /* (hi <= my lane <= 63) */
        }
        NPROF_ADD(1, nt1);
        const uint64_t nt2 = NPROF_T();
        uint64_t nserial = 0;
        for (;;) {
            const uint64_t pm = __ballot(pending);
            if (pm == 0ull) break;
            const int ready = pending && (need & pm) == 0ull;
            const int simple = ready && len <= 16u && dist >= len;
            // (a) short, non-overlapping, source in the tile
            copy_short_match_u(S, simple && src_in_lds, p, len, (uint32_t)src_rel);
            // (a') a short run of one byte (distance 1: 2.8 % of a photo's matches, the commonest kind that is not (a))
            int rle = 0;
            if constexpr (LDS::ES == 1) {
                rle = ready && dist == 1u && len <= 16u && src_in_lds;
                if (rle) {
                    const uint32_t x = (uint32_t)S.tile[p - 1u] * 0x01010101u;
                    st_match_bytes(S, p, len, x, x, x, x);
                }
            }
            // (Measured and not kept: matches of up to 64 bytes from at least 8 bytes back copied by their own lane, eight bytes at
            // a time -- the divergent loop costs the rounds what it saves in one-at-a-time copies: fs_angrymob 20.3 -> 20.8 ms.)
            // (b) everything else: one match at a time, all 64 lanes copy
            unsigned long long gm = __ballot(ready && !(simple && src_in_lds) && !rle);
            const uint64_t nt3 = NPROF_T();
            while (gm) {
                int sl = __ffsll(gm) - 1;
                gm &= gm - 1;
                const uint32_t lp = wave_bcast_u32(p, (uint32_t)sl);
                const uint32_t ll = wave_bcast_u32(len, (uint32_t)sl);
                const uint32_t ld = wave_bcast_u32(dist, (uint32_t)sl);
                if constexpr (LDS::ES == 1) {
                    if (ld == 1u && ll >= 8u && (int64_t)lp - 1 >= lds_rel0) { /* a long run (flat image areas: two thirds of such a
                                                                                  file's matches): eight bytes per lane */
                        const uint32_t x = (uint32_t)S.tile[lp - 1u] * 0x01010101u;
                        const uint32_t at = 8u * lane + 8u <= ll ? 8u * lane : ll - 8u; /* the last word overlaps the one before */
                        if (8u * lane < ll) reinterpret_cast<pk_u64 *>(S.tile + lp + at)->v = ((uint64_t)x << 32) | x;
                        continue;
                    }
                    if (ld >= ll && (int64_t)lp - (int64_t)ld >= lds_rel0) { /* a long copy that does not overlap itself, source in the
                                                                                tile: eight bytes per lane, no run index to compute
                                                                                (ll > 16 here) */
                        const uint32_t at = 8u * lane + 8u <= ll ? 8u * lane : ll - 8u;
                        if (8u * lane < ll) {
                            const uint64_t v = reinterpret_cast<const pk_u64 *>(S.tile + (lp - ld) + at)->v;
                            reinterpret_cast<pk_u64 *>(S.tile + lp + at)->v = v;
                        }
                        continue;
                    }
                }
                lz_copy_match_wave(S, O, lp, ll, ld);
            }
            nserial += NPROF_T() - nt3;
            if (ready) pending = 0;
        }
        NPROF_ADD(2, nt2);
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
        if (lane == 0) S.nprof[3] += nserial;
#else
        (void)nserial;
#endif
    }
}

// (Measured and not kept, profiles/r04_near_group2_ab.txt: TWO matches per lane -- groups of 128, the dependency ranges
// searched in LDS, both matches of a lane copied in the same round.  Fewer rounds, but slower everywhere: fs_angrymob on the
// strand pipeline 20.3 -> 24.1 ms, 4096 x 64 KiB text 0.860 -> 0.911 ms -- the second match's state does not fit the 128
// registers these kernels have, and a round's cost is its instructions as much as its latency.)

// (Measured and not kept, profiles/r04_near_sweep_ab.txt: the near matches of a span as a SWEEP in position order -- 64
// consecutive tile positions at a time, one per lane, each lane following its match's source back through the lanes to
// its left by pointer doubling.  About 55 instructions per 64 bytes whatever the matches look like, but one chain of
// about ten dependent LDS round trips per chunk with nothing to overlap them: no faster on photo-like files (fs_angrymob
// 27.5 vs 28.2 ms) and slower everywhere else (gimp_test 26.5 -> 41.7 ms, 4096 x 64 KiB text 0.874 -> 1.000 ms, 512 x
// 1 MiB text 4.06 -> 5.78 ms).  What it would need is several chunks in flight per wavefront.)

// resolve_matches_groups of inflate_kernel.inc on one wavefront's tile: the near matches of each 2048-element span are
// listed in position order and resolved by near_groups_r
template <class LDS> DEV_INLINE void resolve_matches_groups_u(LDS &S, OutState &O, uint32_t from_rel, uint32_t to_rel)
{
    static_assert(LDS::NW == 1, "one wavefront per tile");
    const uint32_t lane = lane_id();
    wave_local_sync();
    for (uint32_t span = from_rel >> 11; span < ((to_rel + 2047u) >> 11); span++) {
        uint32_t wbase = span * 64u + lane;
        uint32_t w = S.bitmap[wbase];
        uint32_t p0 = wbase * 32u;
        if (p0 + 32u <= from_rel || p0 >= to_rel) w = 0;
        else {
            if (p0 < from_rel) w &= ~0u << (from_rel - p0);
            if (p0 + 32u > to_rel) w &= (1u << (to_rel - p0)) - 1u;
        }
        S.bitmap[wbase] = 0; /* consumed */
        if (!__any(w != 0)) continue; /* no near match starts in this span */
        uint32_t total;
        uint32_t pre = wave_excl_scan_u32((uint32_t)__popc(w), &total);
        {
            uint32_t k = pre, ww = w;
            while (ww) {
                uint32_t bit = (uint32_t)__ffs(ww) - 1u;
                ww &= ww - 1u;
                S.mpos[0][k++] = (uint16_t)(p0 + bit);
            }
        }
        wave_local_sync();
        near_groups_r(S, O, total);
        wave_local_sync(); /* S.mpos is rewritten by the next span */
    }
    wave_local_sync();
}

// value of the neighbouring lane (lane ^ 1): a DPP move, no LDS round trip
#ifdef DEBIG_EMU
#define lane_swap1(v) __shfl_xor((v), 1)
#else
DEV_INLINE uint32_t lane_swap1(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, false);
}
#endif
#ifndef TOK_DEPTH
#define TOK_DEPTH 8 /* token rows in flight per lane (twice: the group being placed + the next); 4 -> 8: config 2 594 -> 603 GB/s (profiles/r03_tok_depth_ab.txt) */
#endif

// a window of the long-segment scan (REC_WIN2, inflate_strand_kernel.inc)
#define REC_WIN2 5
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
#define LZ_PROF_PARAM , uint64_t *prof_acc
#define LZ_PROF_ARG , prof_acc
#else
#define LZ_PROF_PARAM
#define LZ_PROF_ARG
#endif
template <class LDS>
DEV_INLINE void lz_replay_units(LDS &S, OutState &O, const debig_ws_rec &rec, const uint32_t *myrows, uint32_t &status LZ_PROF_PARAM);

// debig_strand_pipe_kernel (inflate_strand_kernel.inc): the scan of a stream runs on one wavefront of the workgroup and
// its LZ77 side on the other, record by record.  The scan wavefront publishes how many records are complete (all
// their stores waited for) in LDS; the LZ77 wavefront polls that count, and reads the records past L1 -- the
// producer is still writing records of the same cache line.
struct LzPipe {
    const volatile uint32_t *produced; /* records published so far */
    const volatile uint32_t *done;     /* the scan is finished: the END record is at index *produced */
};
DEV_INLINE debig_ws_rec lz_read_rec(const debig_ws_rec *p, const LzPipe *pipe)
{
    if (!pipe) return *p;
    debig_ws_rec r;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    uint32_t v[8];
DEV_UNROLL
    for (int k = 0; k < 8; k++) v[k] = ld_hist_u32(w + k); /* served by L2 */
    r.kind = v[0]; r.row = v[1]; r.a = v[2]; r.b = v[3];
    r.c = (uint64_t)v[4] | ((uint64_t)v[5] << 32);
    r.d = (uint64_t)v[6] | ((uint64_t)v[7] << 32);
    return r;
}
// wait until record ri is published (or the scan is done); returns the index to read: ri, or the END record's
DEV_INLINE uint32_t lz_pipe_wait(const LzPipe *pipe, uint32_t ri, int want_end)
{
    if (!pipe) return ri;
    for (;;) {
        const uint32_t p = *pipe->produced, d = *pipe->done;
        const int ready = d || (!want_end && ri < p);
        if (__any(ready)) { /* (wave-uniform; the collective lets the CPU emulator run the other wavefront) */
            if (d && (want_end || ri >= p)) return *pipe->produced;
            return ri;
        }
#ifndef DEBIG_EMU
        __builtin_amdgcn_s_sleep(8);
#endif
    }
}

// The LZ77 side of one stream (CHUNKED = false) or of one chunk task of a large stream (CHUNKED =
// true, inflate_chunk_kernel.inc: output starts at out_start inside the recipient, stored blocks are
// copied here, the result is a status word for the chunk instead of a debig_result).  Returns the
// status; O.outpos is where the output ended.
template <bool CHUNKED, class LDS>
DEV_INLINE uint32_t lz_body(LDS &S, OutState &O, const uint8_t *__restrict__ in_arena, const debig_stream &st,
                            const debig_ws_slot &slot, const debig_ws_rec *__restrict__ recs,
                            const uint32_t *__restrict__ rows, const int64_t out_start, debig_ws_rec *end_rec_out
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
                            , uint64_t *prof_out
#endif
                            , const LzPipe *pipe = nullptr)
{
    PROF_DECL
    const uint32_t lane = lane_id();
    const debig_ws_rec *myrec = recs + slot.rec0;
    const uint32_t *myrows = rows + slot.row0 * 64u;
    O.outpos = out_start;
    O.lds_from = out_start;
    O.tile_base = lz_anchor<LDS>(O.out, out_start);
    for (uint32_t k = lane; k < LDS::MAP_WORDS; k += 64) { S.bitmap[k] = 0; S.farmap[k] = 0; S.pend[k] = 0; }
    if (lane == 0) S.internal_err = 0;
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
    if (lane < 4) S.nprof[lane] = 0;
#endif
    wave_local_sync();

    uint32_t status = DEBIG_OK;
    debig_ws_rec rec;
    for (uint32_t ri = 0;; ri++) {
        rec = lz_read_rec(myrec + lz_pipe_wait(pipe, ri, 0), pipe);
        if (rec.kind == REC_END || status != DEBIG_OK) break;
        if (rec.kind == REC_STORED) {
            lz_flush_all(S, O);
            if (CHUNKED) { /* the scan of a chunk does not know where its output goes: the copy happens here */
                if ((uint64_t)O.outpos + rec.c > O.out_cap) { status = DEBIG_E_OUTPUT_FULL; break; }
                if constexpr (LDS::ES == 2) { /* every stored byte is a literal: {b, b} */
                    const uint8_t *in = in_arena + st.in_off;
                    uint16_t *dw = reinterpret_cast<uint16_t *>(O.out) + O.outpos;
                    for (uint64_t k = lane; k < rec.c; k += 64u) {
                        const uint64_t sb = rec.d + k;
                        const uint32_t b = sb < st.in_len ? in[sb] : 0u; /* bytes behind the input read as zero */
                        dw[k] = (uint16_t)(b * 0x0101u);
                    }
                } else {
                    stored_copy<1>(in_arena + st.in_off, st.in_len, (int64_t)rec.d, O.out + O.outpos, (uint32_t)rec.c);
                }
                wave_mem_fence();
                wave_local_sync();
            }
            O.outpos += (int64_t)rec.c;
            O.lds_from = O.outpos;
            O.tile_base = lz_anchor<LDS>(O.out, O.outpos);
            lz_publish(O); /* (the scan published the record behind a wait for the block's stores) */
            continue;
        }
        if (rec.kind == REC_P2) {
            // decode_png aliasing replay (SURVEY.md Appendix C), as in debig_inflate_kernel
            if (CHUNKED && !(O.outpos > st.p2_s0)) continue; /* recorded for every block of the last chunk */
            lz_flush_all(S, O);
            const int fixed = rec.a != 0;
            const uint32_t *rw = myrows + (size_t)rec.row * 64u;
            int64_t end = O.outpos < (int64_t)st.p2_est ? O.outpos : (int64_t)st.p2_est;
            int64_t s_lo = st.p2_s0 > 0 ? st.p2_s0 : 0;
            uint32_t nent = fixed ? 288u : 19u;
            for (int64_t s = s_lo + lane; s < end; s += 64) {
                uint64_t t = (uint64_t)(s - st.p2_s0);
                uint64_t e = t >> 4;
                uint32_t k = (uint32_t)(t & 15u);
                if (e >= nent) {
                    if constexpr (LDS::ES == 2) reinterpret_cast<uint16_t *>(O.out)[s] = 0;
                    else O.out[s] = 0;
                    continue;
                }
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
                    code = rw[3 * e]; used = rw[3 * e + 1]; l = rw[3 * e + 2];
                }
                uint32_t word = k < 4 ? code : k < 8 ? (uint32_t)e : k < 12 ? used : l;
                const uint32_t pb = (word >> (8 * (k & 3u))) & 255u;
                if constexpr (LDS::ES == 2) reinterpret_cast<uint16_t *>(O.out)[s] = (uint16_t)(pb * 0x0101u);
                else O.out[s] = (uint8_t)pb;
            }
            wave_mem_fence();
            wave_local_sync();
            continue;
        }
        if constexpr (!CHUNKED && LDS::ES == 1) {
            if (rec.kind == REC_WIN2) { /* a window of the long-segment scan: unit by unit */
                lz_replay_units(S, O, rec, myrows, status LZ_PROF_ARG);
                if (status != DEBIG_OK) break;
                if (((rec.a >> 8) & 0xffu) == FL_ERR) status = rec.b;
                continue;
            }
        }
        // ---- REC_WIN: replay the window's tokens through the tile.
        // Two batches of 32 segments.  The tile restarts at the batch's first byte whenever the
        // batch would not fit behind what is already in it, so a batch normally lands in the tile
        // in one piece: matches into earlier output are then "far" (source final in HBM, no
        // ordering constraint), only matches inside the batch need the ordered resolve.
        //   fast replay  (the batch fits the tile and the recipient): every segment is replayed by
        //                a PAIR of lanes -- lane 2k+p takes tokens p, p + 2, ... of segment 32 b + k,
        //                the two swap output lengths through DPP -- no limit checks, no parking:
        //                all 64 lanes busy, about a dozen VALU instructions per token;
        //   general replay (highly compressible data, the last bytes of a tight recipient): one
        //                lane per segment, every token checked against the tile and the recipient.
        const uint32_t used_n = rec.a & 0xffu;
        const uint32_t wflag = (rec.a >> 8) & 0xffu;
        const uint32_t *crow = myrows + (size_t)rec.row * 64u;
        const uint32_t cnt = lane < used_n ? crow[lane] : 0u;
        const uint32_t nsym_l = cnt & 1023u;
        uint32_t wtotal;
        const uint32_t pre = wave_excl_scan_u32(cnt >> 10, &wtotal);
        const int64_t w_out0 = O.outpos;
        // 32-bit window-relative positions in the lanes (a window produces < 2^24 bytes): pre = where
        // my segment's output starts, my_e = where it ends (lanes >= used_n: both wtotal)
        const uint32_t my_e = pre + (cnt >> 10);
        const uint64_t cap_left = O.out_cap > (uint64_t)w_out0 ? O.out_cap - (uint64_t)w_out0 : 0u;
        const uint32_t cap_w = cap_left > 0x7fffffffu ? 0x7fffffffu : (uint32_t)cap_left; /* recipient bytes from w_out0 */
        for (uint32_t s0 = 0; s0 < used_n && status == DEBIG_OK;) {
            // the next batch: as many whole segments (at most 32) as fit a tile in one piece
            const uint32_t b_rel0 = (uint32_t)(O.outpos - w_out0); /* == pre of segment s0 */
            uint32_t nseg;
            {
                const int fit = lane >= s0 && lane < s0 + 32u && lane < used_n &&
                                my_e - b_rel0 <= (uint32_t)LDS::T2 - 16u && my_e <= cap_w;
                const unsigned long long fm = __ballot(fit) >> s0;
                nseg = ~fm == 0ull ? 64u : (uint32_t)(__ffsll(~fm) - 1);
            }
            const int fast = nseg != 0;
            if (!fast) nseg = 1; /* a segment that needs the general replay goes alone */
            int64_t w_out1 = w_out0 + (int64_t)wave_bcast_u32(my_e, s0 + nseg - 1u);
            const uint32_t batch_s0 = s0;
            s0 += nseg;
            // the tile's stores stay in flight while the batch is replayed: the wait comes before the
            // first history read (far copy), behind the replay's own work
            if (fast && w_out1 > O.tile_base + LDS::T2 && O.outpos > O.lds_from) lz_flush_all(S, O, 0);
            if (fast && w_out1 <= O.tile_base + LDS::T2) {
                // ---- fast replay
                PROF_BEGIN();
                const uint32_t p = lane & 1u, pm = 0u - p;
                const int sl = (int)(batch_s0 + (lane >> 1));
                const int active = (lane >> 1) < nseg;
                const uint32_t sn = __shfl(nsym_l, sl & 63);
                const uint32_t s_nsym = active ? sn : 0u;
                uint32_t rel = (uint32_t)(w_out0 - O.tile_base) + __shfl(pre, sl & 63);
                const int32_t tb32 = O.tile_base > 70000 ? 70000 : (int32_t)O.tile_base;
                const int chk_far = tb32 < 32768; /* a distance can only be too far near the start */
                const uint32_t lds_rel = (uint32_t)(O.lds_from - O.tile_base);
                const uint32_t *tp = crow + 64u + (uint32_t)sl + 64u * p; /* my j-th token: tp[128 j] */
                uint32_t my = p;                                            /* its index in the segment */
                uint32_t err_pos = 0xffffffffu;
                uint32_t tc[TOK_DEPTH], tn[TOK_DEPTH];
DEV_UNROLL
                for (uint32_t j = 0; j < TOK_DEPTH; j++) tc[j] = my + 2u * j < s_nsym ? ld_token(tp + 128u * j) : 0u;
                while (__any(my < s_nsym)) {
DEV_UNROLL
                    for (uint32_t j = 0; j < TOK_DEPTH; j++)
                        tn[j] = my + 2u * (TOK_DEPTH + j) < s_nsym ? ld_token(tp + 128u * (TOK_DEPTH + j)) : 0u;
DEV_UNROLL
                    for (uint32_t j = 0; j < TOK_DEPTH; j++) {
                        const uint32_t t = tc[j];
                        const int valid = my < s_nsym;
                        const uint32_t is_len = t >> 31, len3 = (t >> 16) & 0xffu;
                        const uint32_t outlen = valid ? (is_len ? len3 + 3u : 1u) : 0u;
                        const uint32_t pout = lane_swap1(outlen);
                        const uint32_t pos = rel + (pout & pm);
                        rel += outlen + pout;
                        my += 2u;
                        if (valid) {
                            S.tile[pos] = (typename LDS::Elem)(is_len ? len3 : (LDS::ES == 2 ? (t & 255u) * 0x0101u : t));
                            if (is_len) {
                                const uint32_t dm1 = t & 0x7fffu;
                                S.tile[pos + 1] = (typename LDS::Elem)(dm1 & 255u);
                                S.tile[pos + 2] = (typename LDS::Elem)(dm1 >> 8);
                                // src/inflate.c:1843: distance beyond the start of the output
                                if (chk_far && (int32_t)(dm1 + 1u) > tb32 + (int32_t)pos) err_pos = pos < err_pos ? pos : err_pos;
                                uint32_t *map = ((int32_t)(pos + len3 + 3u) - (int32_t)(dm1 + 1u) <= (int32_t)lds_rel) ? S.farmap : S.bitmap;
                                atomicOr(&map[pos >> 5], 1u << (pos & 31u));
                            }
                        }
                    }
DEV_UNROLL
                    for (uint32_t j = 0; j < TOK_DEPTH; j++) tc[j] = tn[j];
                    tp += 128u * TOK_DEPTH;
                }
                PROF_END(0);
                if (chk_far && __any(err_pos != 0xffffffffu)) {
                    status = DEBIG_E_DIST_TOO_FAR; /* the output ends at the first failing token */
                    w_out1 = O.tile_base + (int64_t)wave_min_u32(err_pos);
                }
                const uint32_t from_rel = (uint32_t)(O.outpos - O.tile_base);
                const uint32_t to_rel = (uint32_t)(w_out1 - O.tile_base);
                wave_mem_fence(); /* the flushed tile is history now */
                lz_publish(O);
                wave_local_sync();
                PROF_BEGIN();
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
                continue;
            }
            // ---- general replay: lane L (of the batch) walks segment L's tokens
            const int mine = lane >= batch_s0 && lane < batch_s0 + nseg;
            uint32_t remaining = mine ? nsym_l : 0u;
            int64_t oc = w_out0 + (int64_t)pre;
            const uint32_t *tp = crow + 64u + lane;
            uint32_t lane_err = 0;
            int64_t lane_err_pos = 0;
            for (;;) {
                const int64_t lim = O.tile_base + LDS::T2;
                PROF_BEGIN();
                {
                    uint32_t rel = (uint32_t)(oc - O.tile_base);
                    const int64_t room = (int64_t)O.out_cap - O.tile_base;
                    const uint32_t cap_rel = room > 0x7fffffff ? 0x7fffffffu : (room < 0 ? 0u : (uint32_t)room);
                    const int32_t tb32 = O.tile_base > 70000 ? 70000 : (int32_t)O.tile_base;
                    const uint32_t lds_rel = (uint32_t)(O.lds_from - O.tile_base);
                    const int64_t rel_lim64 = lim - O.tile_base;
                    const uint32_t rel_lim = (oc - O.tile_base) >= rel_lim64 ? 0u : (uint32_t)rel_lim64;
                    while (remaining && rel < rel_lim) {
                        const uint32_t t = ld_token(tp);
                        const uint32_t is_len = t >> 31;
                        const uint32_t len = ((t >> 16) & 0xffu) + 3u;
                        const uint32_t dist = (t & 0x7fffu) + 1u;
                        const uint32_t outlen = is_len ? len : 1u;
                        remaining--;
                        tp += 64;
                        // src/inflate.c:1843 distance beyond the start of the output | the output
                        // would exceed recipient_size
                        const uint32_t too_far = is_len & (uint32_t)((int32_t)dist > tb32 + (int32_t)rel);
                        const uint32_t full = (uint32_t)(rel + outlen > cap_rel);
                        if (too_far | full) {
                            lane_err = too_far ? (uint32_t)DEBIG_E_DIST_TOO_FAR : (uint32_t)DEBIG_E_OUTPUT_FULL;
                            lane_err_pos = O.tile_base + (int64_t)rel;
                            remaining = 0;
                            break;
                        }
                        S.tile[rel] = (typename LDS::Elem)(is_len ? len - 3u : (LDS::ES == 2 ? (t & 255u) * 0x0101u : t));
                        if (is_len) {
                            S.tile[rel + 1] = (typename LDS::Elem)((dist - 1u) & 0xffu);
                            S.tile[rel + 2] = (typename LDS::Elem)((dist - 1u) >> 8);
                            uint32_t *map = ((int32_t)(rel + len) - (int32_t)dist <= (int32_t)lds_rel) ? S.farmap : S.bitmap;
                            atomicOr(&map[rel >> 5], 1u << (rel & 31u));
                        }
                        rel += outlen;
                    }
                    if ((oc - O.tile_base) < rel_lim64) oc = O.tile_base + (int64_t)rel;
                }
                PROF_END(0);
                // an error truncates the window's output at the failing token
                unsigned long long em = __ballot(lane_err != 0);
                if (em) {
                    int el = __ffsll(em) - 1;
                    uint32_t es = __shfl(lane_err, el);
                    int64_t ep = __shfl(lane_err_pos, el);
                    if (status == DEBIG_OK) { status = es; w_out1 = ep; }
                    remaining = 0;
                }
                const int64_t upto = w_out1 < lim ? w_out1 : lim;
                const uint32_t from_rel = (uint32_t)(O.outpos - O.tile_base);
                const uint32_t to_rel = (uint32_t)(upto - O.tile_base);
                wave_local_sync();
                PROF_BEGIN();
                far_copy_u(S, O, from_rel, to_rel);
                PROF_END(1);
                PROF_BEGIN();
                resolve_matches_groups_u(S, O, from_rel, to_rel);
                PROF_END(2);
                if (status != DEBIG_OK) {
                    for (uint32_t k = lane; k < LDS::MAP_WORDS; k += 64) { S.bitmap[k] = 0; S.farmap[k] = 0; }
                    wave_local_sync();
                    O.outpos = upto;
                    break;
                }
                if (w_out1 >= lim) {
                    int64_t min_oc;
                    {
                        int64_t c = remaining ? oc : w_out1;
                        for (uint32_t d = 32; d >= 1; d >>= 1) {
                            int64_t o2 = __shfl_xor(c, (int)d);
                            c = o2 < c ? o2 : c;
                        }
                        min_oc = c < w_out1 ? c : w_out1;
                    }
                    const int64_t carry_end = min_oc > lim ? min_oc : lim;
                    PROF_BEGIN();
                    lz_flush_range(S, O, O.lds_from, lim);
                    PROF_END(3);
                    const uint32_t carry = (uint32_t)(carry_end - lim);
                    typename LDS::Elem cv[5];
DEV_UNROLL
                    for (uint32_t it = 0; it < 5; it++) {
                        uint32_t k = it * 64u + lane;
                        if (k < carry) cv[it] = S.tile[LDS::T2 + k];
                    }
                    wave_local_sync();
DEV_UNROLL
                    for (uint32_t it = 0; it < 5; it++) {
                        uint32_t k = it * 64u + lane;
                        if (k < carry) S.tile[k] = cv[it];
                    }
                    wave_local_sync();
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
        }
        if (status != DEBIG_OK) break;
        if (wflag == FL_ERR) status = rec.b;
    }
    // the scan kernel's verdict comes last in stream order: an error found here wins
    debig_ws_rec endr = rec;
    if (endr.kind != REC_END) {
        if (pipe) {
            endr = lz_read_rec(myrec + lz_pipe_wait(pipe, 0, 1), pipe); /* (after an error: once the scan is done) */
        } else {
            for (uint32_t ri = 0;; ri++) { /* skip to the END record (only after an error) */
                endr = myrec[ri];
                if (endr.kind == REC_END) break;
            }
        }
    }
    if (status == DEBIG_OK) status = endr.a;
    lz_flush_all(S, O);
    *end_rec_out = endr;
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
    prof_acc[6] = __builtin_amdgcn_s_memtime() - prof_start;
    prof_acc[3] = S.nprof[0]; /* (the flush slot is unused: its time is inside the replay) */
    prof_acc[4] = S.nprof[1];
    prof_acc[5] = S.nprof[3];
    prof_acc[7] = S.nprof[2];
    for (int pi = 0; pi < 8; pi++) prof_out[pi] = prof_acc[pi];
#endif
    return status;
}

// the LZ77 side of stream `sid` whose scan left `slot_state` (handed over in a register)
template <class LDS>
DEV_INLINE void lz_stream(LDS &S, const uint32_t sid, const debig_ws_slot &slot, const uint32_t slot_state,
                          uint8_t *__restrict__ out_arena, const debig_stream *__restrict__ streams, debig_result *results,
                          const debig_ws_rec *__restrict__ recs, const uint32_t *__restrict__ rows, const LzPipe *pipe = nullptr,
                          volatile uint32_t *pub = nullptr /* debig_png_fused_kernel: final bytes so far (OutState::pub) */)
{
    const uint32_t lane = lane_id();
    if (slot_state != DEBIG_OK) {
        // not decoded by the scan kernel (workspace share too small, ...): debig_inflate_kernel
        // takes the stream in the DEBIG_CLASS_RETRY launch that follows
        if (lane == 0) {
            debig_result r;
            r.final_size = 0; r.good = 0; r.status = DEBIG_E_RETRY; r.final_set = 0;
            r.n_blocks = 0; r.n_windows = 0; r.n_rounds = 0; r.in_end_bits = 0;
            for (int pi = 0; pi < 8; pi++) r.prof[pi] = 0;
            results[sid] = r;
        }
        return;
    }
    const debig_stream st = streams[sid];
    OutState O;
    O.out = out_arena + st.out_off;
    O.out2 = O.out;
    O.out_cap = st.out_cap;
    O.pub = pub;
    O.pub_cap = st.p2_on ? (st.p2_s0 > 0 ? st.p2_s0 : 0) : 0x7fffffffffffffffll; /* the aliasing replay rewrites what lies behind p2_s0 */
    debig_ws_rec endr;
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
    uint64_t prof[8];
    const uint32_t status = lz_body<false>(S, O, (const uint8_t *)nullptr, st, slot, recs, rows, 0, &endr, prof, pipe);
#else
    const uint32_t status = lz_body<false>(S, O, (const uint8_t *)nullptr, st, slot, recs, rows, 0, &endr, pipe);
#endif
    if (lane == 0) {
        debig_result r;
        r.final_size = (uint64_t)O.outpos;
        r.good = status == DEBIG_OK;
        r.status = status;
        r.final_set = endr.row;
        r.n_blocks = endr.b;
        r.n_windows = (uint32_t)endr.d;
        r.n_rounds = (uint32_t)(endr.d >> 32);
        r.in_end_bits = endr.c;
#if defined(DEBIG_PROFILE) && !defined(DEBIG_EMU)
        /* diagnostic builds: DEBIG_PROFILE_LZ = 1 reports this kernel's phases (0 token replay, 1 far
         * copy, 2 near resolve, 3 flush, 6 total), else the scan kernel's stay in the result */
        const int keep = results[sid].prof[6] != 0 && !DEBIG_PROFILE_LZ;
        if (keep) { for (int pi = 0; pi < 8; pi++) r.prof[pi] = results[sid].prof[pi]; }
        else { for (int pi = 0; pi < 8; pi++) r.prof[pi] = (uint32_t)(prof[pi] >> 4); }
#else
        for (int pi = 0; pi < 8; pi++) r.prof[pi] = 0;
#endif
        results[sid] = r;
    }
}

// ---- both halves in ONE kernel: the wavefront that scanned a stream replays it.  The two halves are
// bound by different things -- the scan by instruction issue, the LZ77 half by the 128-byte lines its
// history gathers pull from HBM (profiles/r03_fetch_calibration.txt, r03_pmc_traffic.txt) -- and as two
// kernels they run one after the other.  Fused, the wavefronts of a SIMD drift apart (stream lengths
// differ), so at any time some are issuing scan instructions while others wait for gathers, and only
// the streams in their LZ77 half compete for L2 with their history windows.  Tokens and records still
// go through the workspace (the same wavefront reads back what it wrote, after a wait for its stores:
// token rows, counts rows and -- record shares being multiples of 128 bytes -- records are never in a
// cache line another wavefront writes).  LDS is the union of the two layouts, registers the maximum.
struct __attribute__((aligned(16))) ScanLzLds {
    union {
        ScanLds s;
        LzLds l;
    };
};

__global__ void __launch_bounds__(64) DEBIG_LZ_ATTRS
debig_scanlz_kernel(const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                    const debig_stream *__restrict__ streams, uint32_t n_streams,
                    const uint32_t *__restrict__ fixed_tabs, debig_ws_slot *__restrict__ slots,
                    debig_ws_rec *__restrict__ recs, uint32_t *__restrict__ rows, debig_result *results)
{
    __shared__ ScanLzLds U;
    if (blockIdx.x >= n_streams) return;
    const uint32_t sid = split_perm(slots, n_streams)[blockIdx.x]; /* the plan kernel's dispatch order */
    const debig_stream st = streams[sid];
    const debig_ws_slot slot = slots[sid];
    uint32_t state = DEBIG_E_RETRY;
    scan_body<false>(U.s, in_arena, out_arena, st, sid, fixed_tabs, slots, recs, rows, results, 0ull, ~0ull, 1, &state);
    wave_mem_fence(); /* tokens, records, stored-block copies: in L2 before anything is read back */
    wave_local_sync();
    lz_stream(U.l, sid, slot, state, out_arena, streams, results, recs, rows);
}

// ---- DEBIG_WAVES_SPLIT_QUEUED: the same two halves behind PERSISTENT workgroups with a work queue, for
// batches whose ORDER mixes cheap and expensive streams.  With one workgroup per stream the hardware
// deals workgroups to the shader engines round-robin BY INDEX, whatever they cost: 4096 fixed-Huffman
// streams alternating with 4096 tiny ones put every Huffman stream on the same half of the chip and took
// 1.67 ms instead of 0.89 (tools/bench_mixed_order.py, profiles/r03_split_order_robustness.txt).  Here
// the launch is as many workgroups as are resident together; workgroup b starts with stream b and then
// takes the next unclaimed stream, in stream order, from a counter in the workspace until none is left.
// The counter is never reset between launches: every workgroup fetches until it is told "none left", so
// a launch adds exactly n to it (n - grid claims + grid refusals), launch k sees the values
// [k n, (k + 1) n) and a fetch is reduced mod n (64 bits: no wrap; the plan kernel zeroes it; a captured
// graph can replay the launch).  Not the default: the loop costs the bodies 44 spilled registers and the
// counter is one address for the whole chip -- a batch sorted by kind (config 2) runs 2-4 % slower.
#ifdef DEBIG_EMU
DEV_INLINE uint64_t queue_fetch_add(uint64_t *p, uint64_t v) { const uint64_t o = *p; *p = o + v; return o; }
#else
DEV_INLINE uint64_t queue_fetch_add(uint64_t *p, uint64_t v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif
__global__ void __launch_bounds__(64) DEBIG_LZ_ATTRS
debig_scanlz_queue_kernel(const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                          const debig_stream *__restrict__ streams, uint32_t n_streams,
                          const uint32_t *__restrict__ fixed_tabs, debig_ws_slot *__restrict__ slots,
                          debig_ws_rec *__restrict__ recs, uint32_t *__restrict__ rows, debig_result *results)
{
    __shared__ ScanLzLds U;
    uint64_t *queue = reinterpret_cast<uint64_t *>(split_queue(slots, n_streams));
    uint32_t sid = blockIdx.x;
    while (sid < n_streams) { /* wave-uniform */
        const debig_stream st = streams[sid];
        const debig_ws_slot slot = slots[sid];
        uint32_t state = DEBIG_E_RETRY;
        scan_body<false>(U.s, in_arena, out_arena, st, sid, fixed_tabs, slots, recs, rows, results, 0ull, ~0ull, 1, &state);
        wave_mem_fence();
        wave_local_sync();
        lz_stream(U.l, sid, slot, state, out_arena, streams, results, recs, rows);
        wave_local_sync();
        uint32_t nx = 0;
        if (lane_id() == 0) nx = gridDim.x + (uint32_t)(queue_fetch_add(queue, 1ull) % n_streams);
        sid = wave_bcast_u32(nx, 0);
    }
}
