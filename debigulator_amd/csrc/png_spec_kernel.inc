// png_spec_kernel.inc -- the general PNG de-filter (include/decode_png.h: debig_png_decode_batch).
//
// Every colour type and bit depth the PNG specification allows, Adam7 passes and tRNS, to RGBA8 (debig_png_spec_defilter_kernel)
// or to any output format of decode_png.h (debig_png_spec_defilter_fmt_kernel, the same body with another store stage; its
// channel-planar form is debig_png_spec_defilter_planar_kernel; debig_png_spec_defilter_index_kernel stores raw labels --
// palette indices and grey samples as stored -- for debig_png_decode_batch_labels).  One TASK is one
// (image, pass) sub-image (debig_png_spec_task); a non-interlaced image is one task placed at (0, 0, 1, 1).
//
// Mapping (what png_kernel.inc measured, generalised to a filter unit of BPP = 1, 2, 3, 4, 6 or 8 bytes):
//   - one workgroup of PNG_SPEC_NWD wavefronts per task; wavefront k takes the bands of 64 rows k, k + NWD, ...;
//   - lane r of a band owns row band*64 + r and runs ONE GROUP of K units (K*BPP = 8, 12 or 16 bytes) behind the row
//     above: the group's "up" bytes are what the lane above produced in the previous macro-step (DPP one-lane shift),
//     "left" and "up-left" are the last unit of the lane's own previous group and of its previous "up";
//   - the row bytes are staged through a padded LDS tile, PNG_SPEC_BLOCK macro-steps per bulk load phase;
//   - the predictors run on packed 2 x 16-bit halves (pk_defilter of png_kernel.inc), one or two dwords per unit;
//   - the first row of a band takes its "up" bytes from the de-filtered last row of the band above, which lane 63 of
//     that band's wavefront stores (raw bytes, not pixels) into a per-task scratch ring of NWD rows; the wavefronts run
//     as a pipeline on LDS progress words, as the NWD template of png_kernel.inc does;
//   - sub-byte unpacking, 16 -> 8 reduction, the tRNS key, the palette lookup and the strided Adam7 store happen
//     after the de-filter, in registers.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_kernel.inc in front of it.

#define PNG_SPEC_NWD 4u
#define PNG_SPEC_BLOCK 8u                         /* macro-steps per load phase                                    */
#define PNG_SPEC_QUADS (PNG_SPEC_BLOCK + 1u)      /* 16 B pieces per row and phase: 8 groups of <= 16 B + alignment */
#define PNG_SPEC_ROW_DW (4u * PNG_SPEC_QUADS)     /* 36 dwords: an odd number of quads, b128 reads conflict-free   */

struct __attribute__((aligned(16))) PngSpecLds {
    uint32_t tile[PNG_SPEC_NWD][64 * PNG_SPEC_ROW_DW]; /* raw row bytes, one row per lane          */
    uint32_t uptile[PNG_SPEC_NWD][PNG_SPEC_BLOCK * 4]; /* lane 0: the de-filtered row above the band */
    uint32_t pal[256];                                 /* RGBA, tRNS alpha folded in                 */
    uint32_t progress[PNG_SPEC_NWD];                   /* band * (ngroups + 1) + groups of its last row in the scratch ring */
    uint32_t first_bad;                                /* first row whose filter byte is > 4         */
    uint32_t pal_bad;                                  /* a palette index >= the number of entries   */
};

// units per group: 8..16 bytes, a multiple of 4 (the scratch row and the tile are addressed in dwords)
template <int BPP> struct PngSpecShape {
    static constexpr uint32_t K = BPP == 1 ? 8u : BPP <= 4 ? 4u : 2u;
    static constexpr uint32_t GB = K * (uint32_t)BPP; /* bytes per group: 8, 8, 12, 16, 12, 16 */
    static constexpr uint32_t GD = GB / 4u;           /* dwords per group                      */
    static constexpr uint32_t ND = BPP > 4 ? 2u : 1u; /* dwords per unit                       */
};

// nb (<= 4) bytes at byte offset off of the dword array d (d has one dword of padding)
DEV_INLINE uint32_t spec_get(const uint32_t *d, uint32_t off, uint32_t nb)
{
    const uint32_t w = off >> 2, s = off & 3u;
    const uint32_t x = s ? (d[w] >> (8u * s)) | (d[w + 1] << (32u - 8u * s)) : d[w];
    return nb >= 4u ? x : x & ((1u << (8u * nb)) - 1u);
}
DEV_INLINE void spec_put(uint32_t *d, uint32_t off, uint32_t v)
{
    const uint32_t w = off >> 2, s = off & 3u;
    d[w] |= v << (8u * s);
    if (s) d[w + 1] |= v >> (32u - 8u * s);
}

// one group, serial in x: a = my previous unit, c = the previous "up" unit (both carried from group to group)
template <int BPP, int FT>
DEV_INLINE void spec_defilter_group(const uint32_t *v, const uint32_t *u, uint32_t *a, uint32_t *c, uint32_t *r)
{
    typedef PngSpecShape<BPP> S;
DEV_UNROLL
    for (uint32_t i = 0; i <= S::GD; i++) r[i] = 0u;
DEV_UNROLL
    for (uint32_t j = 0; j < S::K; j++) {
DEV_UNROLL
        for (uint32_t d = 0; d < S::ND; d++) {
            const uint32_t off = j * (uint32_t)BPP + 4u * d;
            const uint32_t nb = (uint32_t)BPP - 4u * d < 4u ? (uint32_t)BPP - 4u * d : 4u;
            const uint32_t vb = spec_get(v, off, nb), ub = spec_get(u, off, nb);
            const PkPx x = pk_defilter<FT>(pk_split(vb), pk_split(a[d]), pk_split(ub), pk_split(c[d]));
            a[d] = pk_join(x);
            c[d] = ub;
            spec_put(r, off, a[d]);
        }
    }
}

// one pixel of a unit of >= 8-bit samples (bytes in stream order, lo = bytes 0..3, hi = bytes 4..7)
DEV_INLINE uint32_t spec_pixel(uint32_t lo, uint32_t hi, uint32_t ct, uint32_t depth, const debig_png_spec_task &t,
                               const uint32_t *pal, uint32_t &pal_bad)
{
    const uint32_t b0 = lo & 0xffu, b1 = (lo >> 8) & 0xffu, b2 = (lo >> 16) & 0xffu, b3 = lo >> 24;
    const uint32_t b4 = hi & 0xffu, b5 = (hi >> 8) & 0xffu, b6 = (hi >> 16) & 0xffu;
    if (depth == 16u) {
        if (ct == 0u) {
            const uint32_t a = t.has_key && ((b0 << 8) | b1) == t.key[0] ? 0u : 255u;
            return b0 * 0x010101u | (a << 24);
        }
        if (ct == 2u) {
            const uint32_t a = t.has_key && ((b0 << 8) | b1) == t.key[0] && ((b2 << 8) | b3) == t.key[1] &&
                                       ((b4 << 8) | b5) == t.key[2] ? 0u : 255u;
            return b0 | (b2 << 8) | (b4 << 16) | (a << 24);
        }
        if (ct == 4u) return b0 * 0x010101u | (b2 << 24);
        return b0 | (b2 << 8) | (b4 << 16) | (b6 << 24); /* 6 */
    }
    if (ct == 0u) {
        const uint32_t a = t.has_key && b0 == t.key[0] ? 0u : 255u;
        return b0 * 0x010101u | (a << 24);
    }
    if (ct == 2u) {
        const uint32_t a = t.has_key && b0 == t.key[0] && b1 == t.key[1] && b2 == t.key[2] ? 0u : 255u;
        return b0 | (b1 << 8) | (b2 << 16) | (a << 24);
    }
    if (ct == 3u) {
        pal_bad |= b0 >= t.n_pal;
        return pal[b0];
    }
    if (ct == 4u) return b0 * 0x010101u | (b1 << 24);
    return lo; /* 6 */
}
// one pixel of a 1-, 2- or 4-bit sample (colour types 0 and 3)
DEV_INLINE uint32_t spec_pixel_sub(uint32_t s, uint32_t ct, uint32_t depth, const debig_png_spec_task &t, const uint32_t *pal,
                                   uint32_t &pal_bad)
{
    if (ct == 3u) {
        pal_bad |= s >= t.n_pal;
        return pal[s];
    }
    const uint32_t g = s * (depth == 1u ? 255u : depth == 2u ? 85u : 17u);
    const uint32_t a = t.has_key && s == t.key[0] ? 0u : 255u;
    return g * 0x010101u | (a << 24);
}

// RGBA8 (debig_png_spec_defilter_kernel): one dword per pixel, stored pixel by pixel (the code is in png_spec_task)
struct PngSpecOutRgba8 {};
DEV_INLINE uint32_t spec_out_bytes(PngSpecOutRgba8, const debig_png_spec_task &) { return 4u; }
constexpr bool spec_out_rgba8(PngSpecOutRgba8) { return true; }

// Any output format (debig_png_spec_defilter_fmt_kernel, t.out_fmt: include/decode_png.h DEBIG_PNG_FMT_*, resolved):
// layout RGBA / RGB / GRAY / GRAY_ALPHA (bits 0..1), 16-bit little-endian samples (DEBIG_PNG_FMT_16 = 0x10) or 8-bit.
// A pixel is first built as four 16-bit samples (8-bit sources times 257), then reduced to the output depth (the high
// byte), then laid out: Y = (6968 R + 23434 G + 2366 B + 16384) >> 15 on the output-depth samples (the identity on grey
// sources, where R = G = B), alpha dropped or kept.
struct PngSpecOutFmt {};
constexpr bool spec_out_rgba8(PngSpecOutFmt) { return false; }
struct SpecPx16 { uint32_t r, g, b, a; };
DEV_INLINE uint32_t spec_fmt_bytes(uint32_t f)
{
    const uint32_t lay = f & 3u;
    return (lay == 0u ? 4u : lay == 1u ? 3u : lay == 2u ? 1u : 2u) << ((f >> 4) & 1u);
}
DEV_INLINE uint32_t spec_out_bytes(PngSpecOutFmt, const debig_png_spec_task &t) { return spec_fmt_bytes(t.out_fmt); }

// spec_pixel at full depth
DEV_INLINE SpecPx16 spec_pixel16(uint32_t lo, uint32_t hi, uint32_t ct, uint32_t depth, const debig_png_spec_task &t,
                                 const uint32_t *pal, uint32_t &pal_bad)
{
    SpecPx16 p;
    if (depth == 16u) {
        const uint32_t s0 = ((lo & 0xffu) << 8) | ((lo >> 8) & 0xffu), s1 = ((lo >> 8) & 0xff00u) | (lo >> 24);
        const uint32_t s2 = ((hi & 0xffu) << 8) | ((hi >> 8) & 0xffu), s3 = ((hi >> 8) & 0xff00u) | (hi >> 24);
        if (ct == 0u || ct == 4u) {
            p.r = p.g = p.b = s0;
            p.a = ct == 4u ? s1 : t.has_key && s0 == t.key[0] ? 0u : 0xffffu;
        } else {
            p.r = s0; p.g = s1; p.b = s2;
            p.a = ct == 6u ? s3 : t.has_key && s0 == t.key[0] && s1 == t.key[1] && s2 == t.key[2] ? 0u : 0xffffu;
        }
        return p;
    }
    const uint32_t b0 = lo & 0xffu, b1 = (lo >> 8) & 0xffu, b2 = (lo >> 16) & 0xffu, b3 = lo >> 24;
    if (ct == 3u) {
        pal_bad |= b0 >= t.n_pal;
        const uint32_t e = pal[b0];
        p.r = (e & 0xffu) * 257u; p.g = ((e >> 8) & 0xffu) * 257u; p.b = ((e >> 16) & 0xffu) * 257u; p.a = (e >> 24) * 257u;
    } else if (ct == 0u || ct == 4u) {
        p.r = p.g = p.b = b0 * 257u;
        p.a = ct == 4u ? b1 * 257u : t.has_key && b0 == t.key[0] ? 0u : 0xffffu;
    } else {
        p.r = b0 * 257u; p.g = b1 * 257u; p.b = b2 * 257u;
        p.a = ct == 6u ? b3 * 257u : t.has_key && b0 == t.key[0] && b1 == t.key[1] && b2 == t.key[2] ? 0u : 0xffffu;
    }
    return p;
}
// spec_pixel_sub at full depth
DEV_INLINE SpecPx16 spec_pixel16_sub(uint32_t s, uint32_t ct, uint32_t depth, const debig_png_spec_task &t,
                                     const uint32_t *pal, uint32_t &pal_bad)
{
    SpecPx16 p;
    if (ct == 3u) {
        pal_bad |= s >= t.n_pal;
        const uint32_t e = pal[s];
        p.r = (e & 0xffu) * 257u; p.g = ((e >> 8) & 0xffu) * 257u; p.b = ((e >> 16) & 0xffu) * 257u; p.a = (e >> 24) * 257u;
        return p;
    }
    p.r = p.g = p.b = s * (depth == 1u ? 65535u : depth == 2u ? 21845u : 4369u); /* (255, 85, 17) * 257 */
    p.a = t.has_key && s == t.key[0] ? 0u : 0xffffu;
    return p;
}
// the pixel's bytes in output order, little-endian: lo = bytes 0..3, hi = bytes 4..7
template <uint32_t F>
DEV_INLINE void spec_fmt_pack(SpecPx16 p, uint32_t &lo, uint32_t &hi)
{
    constexpr uint32_t lay = F & 3u;
    constexpr uint32_t sh = F & 0x10u ? 0u : 8u;
    const uint32_t r = p.r >> sh, g = p.g >> sh, b = p.b >> sh, a = p.a >> sh;
    const uint32_t y = (6968u * r + 23434u * g + 2366u * b + 16384u) >> 15;
    if (F & 0x10u) {
        lo = lay <= 1u ? r | (g << 16) : lay == 2u ? y : y | (a << 16);
        hi = lay == 0u ? b | (a << 16) : lay == 1u ? b : 0u;
    } else {
        lo = lay == 0u ? r | (g << 8) | (b << 16) | (a << 24) : lay == 1u ? r | (g << 8) | (b << 16) : lay == 2u ? y : y | (a << 8);
        hi = 0u;
    }
}
// one pixel of PB bytes at p (p is aligned to PB for PB = 1, 2, 4, 8 and to 2 for PB = 6)
template <uint32_t PB>
DEV_INLINE void spec_store_px(uint8_t *p, uint32_t lo, uint32_t hi)
{
    if (PB == 1u) {
        *p = (uint8_t)lo;
    } else if (PB == 2u) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)lo;
    } else if (PB == 3u) {
        p[0] = (uint8_t)lo; p[1] = (uint8_t)(lo >> 8); p[2] = (uint8_t)(lo >> 16);
    } else if (PB == 4u) {
        *reinterpret_cast<uint32_t *>(p) = lo;
    } else if (PB == 6u) {
        uint16_t *q = reinterpret_cast<uint16_t *>(p);
        q[0] = (uint16_t)lo; q[1] = (uint16_t)(lo >> 16); q[2] = (uint16_t)hi;
    } else {
        uint2 v;
        v.x = lo; v.y = hi;
        *reinterpret_cast<uint2 *>(p) = v;
    }
}
// NB contiguous bytes (B: NB / 4 dwords, rounded up) at p, in the widest stores p's alignment allows
template <uint32_t NB>
DEV_INLINE void spec_store_run(uint8_t *p, const uint32_t *B)
{
    const uint32_t al = (uint32_t)reinterpret_cast<uintptr_t>(p) & 15u;
    if (NB % 16u == 0u && al == 0u) {
DEV_UNROLL
        for (uint32_t i = 0; i < NB / 16u; i++) {
            uint4 v;
            v.x = B[4u * i]; v.y = B[4u * i + 1u]; v.z = B[4u * i + 2u]; v.w = B[4u * i + 3u];
            *reinterpret_cast<uint4 *>(p + 16u * i) = v;
        }
    } else if (NB % 8u == 0u && (al & 7u) == 0u) {
DEV_UNROLL
        for (uint32_t i = 0; i < NB / 8u; i++) {
            uint2 v;
            v.x = B[2u * i]; v.y = B[2u * i + 1u];
            *reinterpret_cast<uint2 *>(p + 8u * i) = v;
        }
    } else if (NB % 4u == 0u && (al & 3u) == 0u) {
DEV_UNROLL
        for (uint32_t i = 0; i < NB / 4u; i++) *reinterpret_cast<uint32_t *>(p + 4u * i) = B[i];
    } else if (NB % 2u == 0u && (al & 1u) == 0u) {
DEV_UNROLL
        for (uint32_t i = 0; i < NB / 2u; i++) *reinterpret_cast<uint16_t *>(p + 2u * i) = (uint16_t)(B[i / 2u] >> (16u * (i & 1u)));
    } else {
DEV_UNROLL
        for (uint32_t i = 0; i < NB; i++) p[i] = (uint8_t)(B[i / 4u] >> (8u * (i & 3u)));
    }
}
// N pixels (lo / hi) that belong at x, x + dx, ...: one run when they are contiguous and all inside the row, else
// pixel by pixel up to the row's end
template <uint32_t PB, uint32_t N>
DEV_INLINE void spec_store_pixels(uint8_t *orow, uint64_t x, uint32_t w, uint64_t ostep, uint32_t dx, const uint32_t *lo,
                                  const uint32_t *hi)
{
    if (dx == 1u && x + N <= w) {
        uint32_t B[(N * PB + 3u) / 4u + 1u];
DEV_UNROLL
        for (uint32_t i = 0; i < (N * PB + 3u) / 4u + 1u; i++) B[i] = 0u;
DEV_UNROLL
        for (uint32_t j = 0; j < N; j++) {
            spec_put(B, j * PB, lo[j]);
            if (PB > 4u) spec_put(B, j * PB + 4u, hi[j]);
        }
        spec_store_run<N * PB>(orow + x * PB, B);
    } else {
DEV_UNROLL
        for (uint32_t j = 0; j < N; j++)
            if (x + j < w) spec_store_px<PB>(orow + (x + j) * ostep, lo[j], hi[j]);
    }
}
// Channel-planar (debig_png_spec_defilter_planar_kernel): the same N pixels, channel c of each in plane c.  Here orow is
// the pixel row in plane 0 and ostep the step of one sub-image pixel, both counted in bytes of ONE sample; plane is the
// size of a plane in bytes.  Contiguous pixels inside the row are N consecutive samples in every plane: one run per plane
// (a plane's base is only sample-aligned, so spec_store_run picks the width by the address); else sample by sample up to
// the row's end.
template <uint32_t F, uint32_t N>
DEV_INLINE void spec_store_planar(uint8_t *orow, uint64_t plane, uint64_t x, uint32_t w, uint64_t ostep, uint32_t dx,
                                  const uint32_t *lo, const uint32_t *hi)
{
    constexpr uint32_t CH = (F & 3u) == 0u ? 4u : (F & 3u) == 1u ? 3u : (F & 3u) == 2u ? 1u : 2u, BS = F & 0x10u ? 2u : 1u;
    const bool run = dx == 1u && x + N <= w;
DEV_UNROLL
    for (uint32_t c = 0; c < CH; c++) {
        uint8_t *p = orow + c * plane;
        uint32_t s[N];
DEV_UNROLL
        for (uint32_t j = 0; j < N; j++)
            s[j] = BS == 2u ? ((c < 2u ? lo[j] : hi[j]) >> (16u * (c & 1u))) & 0xffffu : (lo[j] >> (8u * c)) & 0xffu;
        if (run) {
            uint32_t B[(N * BS + 3u) / 4u];
DEV_UNROLL
            for (uint32_t i = 0; i < (N * BS + 3u) / 4u; i++) B[i] = 0u;
DEV_UNROLL
            for (uint32_t j = 0; j < N; j++) B[j * BS / 4u] |= s[j] << (8u * ((j * BS) & 3u));
            spec_store_run<N * BS>(p + x * BS, B);
        } else {
DEV_UNROLL
            for (uint32_t j = 0; j < N; j++)
                if (x + j < w) spec_store_px<BS>(p + (x + j) * ostep, s[j], 0u);
        }
    }
}
template <int BPP, uint32_t F, uint32_t DEPTH, bool PL>
DEV_INLINE void spec_fmt_group_sub(const uint32_t *R, int g, uint32_t w, uint32_t ct, const debig_png_spec_task &t,
                                   const uint32_t *pal, uint32_t &pal_bad, uint8_t *orow, uint64_t ostep, uint64_t plane)
{
    constexpr uint32_t K = PngSpecShape<BPP>::K, CH = (F & 3u) == 0u ? 4u : (F & 3u) == 1u ? 3u : (F & 3u) == 2u ? 1u : 2u;
    constexpr uint32_t PPB = 8u / DEPTH, PB = CH << ((F >> 4) & 1u);
DEV_UNROLL
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t byte = spec_get(R, j, 1u);
        const uint64_t xb = ((uint64_t)g * K + j) * PPB;
        if (xb >= w) break;
        uint32_t lo[PPB], hi[PPB];
DEV_UNROLL
        for (uint32_t s = 0; s < PPB; s++) {
            uint32_t bad = 0u;
            const SpecPx16 p = spec_pixel16_sub((byte >> (8u - DEPTH * (s + 1u))) & ((1u << DEPTH) - 1u), ct, DEPTH, t, pal, bad);
            pal_bad |= xb + s < w ? bad : 0u;
            spec_fmt_pack<F>(p, lo[s], hi[s]);
        }
        if constexpr (PL) spec_store_planar<F, PPB>(orow, plane, xb, w, ostep, t.dx, lo, hi);
        else spec_store_pixels<PB, PPB>(orow, xb, w, ostep, t.dx, lo, hi);
    }
}
template <int BPP, uint32_t F, bool PL>
DEV_INLINE void spec_fmt_group(const uint32_t *R, int g, uint32_t w, uint32_t depth, uint32_t ct, const debig_png_spec_task &t,
                               const uint32_t *pal, uint32_t &pal_bad, uint8_t *orow, uint64_t ostep, uint64_t plane)
{
    constexpr uint32_t K = PngSpecShape<BPP>::K, CH = (F & 3u) == 0u ? 4u : (F & 3u) == 1u ? 3u : (F & 3u) == 2u ? 1u : 2u;
    constexpr uint32_t PB = CH << ((F >> 4) & 1u);
    if (BPP == 1 && depth < 8u) {
        if (depth == 1u) spec_fmt_group_sub<BPP, F, 1u, PL>(R, g, w, ct, t, pal, pal_bad, orow, ostep, plane);
        else if (depth == 2u) spec_fmt_group_sub<BPP, F, 2u, PL>(R, g, w, ct, t, pal, pal_bad, orow, ostep, plane);
        else spec_fmt_group_sub<BPP, F, 4u, PL>(R, g, w, ct, t, pal, pal_bad, orow, ostep, plane);
        return;
    }
    const uint64_t x = (uint64_t)g * K;
    uint32_t lo[K], hi[K];
DEV_UNROLL
    for (uint32_t j = 0; j < K; j++) {
        uint32_t bad = 0u;
        const uint32_t ulo = spec_get(R, j * (uint32_t)BPP, BPP < 4 ? (uint32_t)BPP : 4u);
        const uint32_t uhi = BPP > 4 ? spec_get(R, j * (uint32_t)BPP + 4u, (uint32_t)BPP - 4u) : 0u;
        const SpecPx16 p = spec_pixel16(ulo, uhi, ct, depth, t, pal, bad);
        pal_bad |= x + j < w ? bad : 0u;
        spec_fmt_pack<F>(p, lo[j], hi[j]);
    }
    if constexpr (PL) spec_store_planar<F, K>(orow, plane, x, w, ostep, t.dx, lo, hi);
    else spec_store_pixels<PB, K>(orow, x, w, ostep, t.dx, lo, hi);
}
template <int BPP, bool PL>
DEV_INLINE void spec_fmt_switch(const uint32_t *R, int g, uint32_t w, uint32_t depth, uint32_t ct, const debig_png_spec_task &t,
                                const uint32_t *pal, uint32_t &pal_bad, uint8_t *orow, uint64_t ostep, uint64_t plane)
{
    switch (t.out_fmt) { /* workgroup-uniform */
    case 0x01u: spec_fmt_group<BPP, 0x01u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    case 0x02u: spec_fmt_group<BPP, 0x02u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    case 0x03u: spec_fmt_group<BPP, 0x03u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    case 0x10u: spec_fmt_group<BPP, 0x10u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    case 0x11u: spec_fmt_group<BPP, 0x11u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    case 0x12u: spec_fmt_group<BPP, 0x12u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    case 0x13u: spec_fmt_group<BPP, 0x13u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    default: spec_fmt_group<BPP, 0x00u, PL>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane); break;
    }
}
template <int BPP>
DEV_INLINE void spec_out_group(PngSpecOutFmt, const uint32_t *R, int g, uint32_t w, uint32_t depth, uint32_t ct,
                               const debig_png_spec_task &t, const uint32_t *pal, uint32_t &pal_bad, uint8_t *orow,
                               uint64_t ostep)
{
    spec_fmt_switch<BPP, false>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, 0u);
}

// Channel-planar output (debig_png_spec_defilter_planar_kernel): the pixels of PngSpecOutFmt, built by the same code, stored
// as planes of img_height * img_width samples, one channel after the other without padding.  orow and ostep count in
// samples here (spec_out_bytes is the size of ONE sample); the task carries the full image's height for the plane size.
struct PngSpecOutPlanar {};
constexpr bool spec_out_rgba8(PngSpecOutPlanar) { return false; }
DEV_INLINE uint32_t spec_out_bytes(PngSpecOutPlanar, const debig_png_spec_task &t) { return 1u << ((t.out_fmt >> 4) & 1u); }
template <int BPP>
DEV_INLINE void spec_out_group(PngSpecOutPlanar, const uint32_t *R, int g, uint32_t w, uint32_t depth, uint32_t ct,
                               const debig_png_spec_task &t, const uint32_t *pal, uint32_t &pal_bad, uint8_t *orow,
                               uint64_t ostep)
{
    const uint64_t plane = ((uint64_t)t.img_height * t.img_width) << ((t.out_fmt >> 4) & 1u);
    spec_fmt_switch<BPP, true>(R, g, w, depth, ct, t, pal, pal_bad, orow, ostep, plane);
}

// Raw labels (debig_png_spec_defilter_index_kernel, behind debig_png_decode_batch_labels of decode_png.h): colour types 3 and 0
// only, hence BPP 1 (depths 1..8) or 2 (16-bit grey).  One ELEMENT per pixel -- the palette index or the grey sample as the
// file stores it, nothing scaled, PLTE colours and tRNS unused -- of one byte for depths up to 8 and one little-endian uint16
// for depth 16 (spec_out_bytes is the element).  Sub-byte samples are unpacked MSB first by constant shifts; where dx == 1 the
// elements of a byte (depth < 8) or of the whole group go out as one run (spec_store_pixels), else one by one at the Adam7
// stride.  The palette is never read: only n_pal bounds the index (pal_bad, as in the other policies).
struct PngSpecOutIndex {};
constexpr bool spec_out_rgba8(PngSpecOutIndex) { return false; }
DEV_INLINE uint32_t spec_out_bytes(PngSpecOutIndex, const debig_png_spec_task &t) { return t.depth == 16u ? 2u : 1u; }
template <uint32_t DEPTH>
DEV_INLINE void spec_index_group_sub(const uint32_t *R, int g, uint32_t w, uint32_t lim, uint32_t dx, uint32_t &pal_bad,
                                     uint8_t *orow, uint64_t ostep)
{
    constexpr uint32_t K = PngSpecShape<1>::K, PPB = 8u / DEPTH;
DEV_UNROLL
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t byte = spec_get(R, j, 1u);
        const uint64_t xb = ((uint64_t)g * K + j) * PPB;
        if (xb >= w) break;
        uint32_t s[PPB];
DEV_UNROLL
        for (uint32_t k = 0; k < PPB; k++) {
            s[k] = (byte >> (8u - DEPTH * (k + 1u))) & ((1u << DEPTH) - 1u);
            pal_bad |= xb + k < w && s[k] >= lim ? 1u : 0u;
        }
        spec_store_pixels<1u, PPB>(orow, xb, w, ostep, dx, s, s);
    }
}
template <int BPP>
DEV_INLINE void spec_out_group(PngSpecOutIndex, const uint32_t *R, int g, uint32_t w, uint32_t depth, uint32_t ct,
                               const debig_png_spec_task &t, const uint32_t *, uint32_t &pal_bad, uint8_t *orow, uint64_t ostep)
{
    static_assert(BPP == 1 || BPP == 2, "labels are one sample of at most 16 bits per pixel");
    constexpr uint32_t K = PngSpecShape<BPP>::K;
    const uint32_t lim = ct == 3u ? t.n_pal : 0x10000u; /* grey samples have no bound */
    if (BPP == 1 && depth < 8u) {
        if (depth == 1u) spec_index_group_sub<1u>(R, g, w, lim, t.dx, pal_bad, orow, ostep);
        else if (depth == 2u) spec_index_group_sub<2u>(R, g, w, lim, t.dx, pal_bad, orow, ostep);
        else spec_index_group_sub<4u>(R, g, w, lim, t.dx, pal_bad, orow, ostep);
        return;
    }
    const uint64_t x = (uint64_t)g * K;
    uint32_t s[K];
DEV_UNROLL
    for (uint32_t j = 0; j < K; j++) {
        const uint32_t u = spec_get(R, j * (uint32_t)BPP, (uint32_t)BPP);
        s[j] = BPP == 2 ? ((u & 0xffu) << 8) | (u >> 8) : u; /* the stream is big-endian */
        pal_bad |= x + j < w && s[j] >= lim ? 1u : 0u;
    }
    spec_store_pixels<(uint32_t)BPP, K>(orow, x, w, ostep, t.dx, s, s);
}

template <int BPP, class O>
DEV_INLINE void png_spec_task(PngSpecLds &L, uint8_t *__restrict__ arena, uint8_t *__restrict__ rgba_arena,
                              const debig_png_spec_task &t, const uint32_t tid)
{
    typedef PngSpecShape<BPP> S;
    constexpr uint32_t K = S::K, GB = S::GB, GD = S::GD, ND = S::ND;
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    uint32_t *tile = &L.tile[wv][lane * PNG_SPEC_ROW_DW];
    uint32_t *uptile = L.uptile[wv];
    const uint32_t w = t.width, h = t.height, ct = t.color_type, depth = t.depth;
    const uint64_t rowb = ((uint64_t)w * t.channels * depth + 7u) / 8u;
    const uint32_t ngroups = (uint32_t)((rowb + GB - 1u) / GB);
    const uint32_t ppb = depth < 8u ? 8u / depth : 1u; /* pixels per byte (sub-byte samples) */
    const uint64_t base_al = t.stream_off & ~(uint64_t)3;
    const uint8_t *sbase = arena + base_al;
    const int64_t stream_len_al = (int64_t)(t.stream_off & 3u) + (int64_t)h * (int64_t)(rowb + 1u);
    const uint64_t pitch = ((uint64_t)ngroups * GB + 15u) & ~(uint64_t)15u; /* scratch ring: one row per wavefront */
    uint32_t *ring = reinterpret_cast<uint32_t *>(arena + t.scratch_off);
    uint8_t *out = rgba_arena + t.rgba_off;
    uint32_t pal_bad = 0;
    for (uint32_t band = wv; (uint64_t)band * 64u < h; band += PNG_SPEC_NWD) {
        if (__any(*(volatile uint32_t *)&L.first_bad != 0xffffffffu)) break; /* another wavefront failed the image */
        const uint32_t row = band * 64u + lane;
        const int active = row < h;
        const int64_t rs = (int64_t)(t.stream_off & 3u) + (int64_t)(active ? row : 0u) * (int64_t)(rowb + 1u); /* filter byte */
        const uint32_t ft = active ? (uint32_t)sbase[rs] : 0u;
        const unsigned long long badm = __ballot(active && ft > 4u);
        if (badm) {
            if (lane == 0) atomicMin(&L.first_bad, band * 64u + (uint32_t)(__ffsll(badm) - 1));
            break;
        }
        const uint32_t row_sh = (uint32_t)((rs + 1) & 3);
        const uint32_t *upring = ring + (pitch / 4u) * ((band + PNG_SPEC_NWD - 1u) % PNG_SPEC_NWD);
        uint32_t *myring = ring + (pitch / 4u) * (band % PNG_SPEC_NWD);
        const uint64_t out_y = (uint64_t)t.y0 + (uint64_t)(active ? row : 0u) * t.dy;
        uint8_t *orow = out + (out_y * t.img_width + t.x0) * spec_out_bytes(O(), t);
        const uint64_t ostep = spec_out_bytes(O(), t) * (uint64_t)t.dx;
        uint32_t R[GD + 1], a[ND], c[ND];
DEV_UNROLL
        for (uint32_t i = 0; i <= GD; i++) R[i] = 0u;
DEV_UNROLL
        for (uint32_t d = 0; d < ND; d++) a[d] = c[d] = 0u;
        const uint32_t nsteps = ngroups + 63u;
        int stop = 0;
        for (uint32_t T0 = 0; T0 < nsteps && !stop; T0 += PNG_SPEC_BLOCK) {
            png_wave_sync<(int)PNG_SPEC_NWD>();
            if (band > 0) {
                // the groups [T0, T0 + BLOCK) of the row above my band must be in the ring: poll its producer
                const uint32_t prod = (wv + PNG_SPEC_NWD - 1u) % PNG_SPEC_NWD;
                const uint32_t need_g = T0 + PNG_SPEC_BLOCK < ngroups ? T0 + PNG_SPEC_BLOCK : ngroups;
                const uint32_t need = (band - 1u) * (ngroups + 1u) + need_g;
                uint32_t spins = 0, fbv = 0xffffffffu;
                for (;;) {
                    const uint32_t have = *(volatile uint32_t *)&L.progress[prod];
                    fbv = *(volatile uint32_t *)&L.first_bad;
                    const int done = have >= need || fbv != 0xffffffffu || ++spins > (1u << 24);
                    if (__all(done)) break;
#ifndef DEBIG_EMU
                    __builtin_amdgcn_s_sleep(4);
#endif
                }
                const int timed_out = spins > (1u << 24);
                if (__any(fbv != 0xffffffffu) || timed_out) {
                    if (timed_out && lane == 0) atomicMin(&L.first_bad, 0xfffffffeu); /* internal guard: fail the image */
                    stop = 1;
                    continue;
                }
            }
            {
                // my row's groups T0 - lane .. + BLOCK - 1 as 16 B pieces; pieces that hold none of the bytes I need are 0
                const int64_t gbase = (int64_t)T0 - (int64_t)lane;
                const int64_t need_lo = rs + 1 + (gbase > 0 ? gbase : 0) * (int64_t)GB;
                const int64_t o0 = (rs + 1 + gbase * (int64_t)GB) & ~(int64_t)3;
                PngQuad q[PNG_SPEC_QUADS];
                uint32_t okm = 0;
DEV_UNROLL
                for (uint32_t c4 = 0; c4 < PNG_SPEC_QUADS; c4++) {
                    const int64_t po = o0 + 16 * (int64_t)c4;
                    const int ok = active && po + 16 > need_lo && po < stream_len_al;
                    okm |= (uint32_t)ok << c4;
                    q[c4] = png_ld_quad<false>(sbase + (ok ? po : rs));
                }
                PNG_ISSUE_BARRIER();
DEV_UNROLL
                for (uint32_t c4 = 0; c4 < PNG_SPEC_QUADS; c4++) {
                    const int ok = (int)((okm >> c4) & 1u);
                    uint4 v;
                    v.x = ok ? q[c4].x : 0u; v.y = ok ? q[c4].y : 0u; v.z = ok ? q[c4].z : 0u; v.w = ok ? q[c4].w : 0u;
                    *reinterpret_cast<uint4 *>(&tile[4u * c4]) = v;
                }
                if (band > 0 && lane < PNG_SPEC_BLOCK) { /* lane 0's "up" groups T0 .. T0 + BLOCK - 1 */
                    const uint32_t gq = T0 + lane;
DEV_UNROLL
                    for (uint32_t i = 0; i < GD; i++) uptile[lane * GD + i] = gq < ngroups ? ld_hist_u32(upring + gq * GD + i) : 0u;
                }
            }
            png_wave_sync<(int)PNG_SPEC_NWD>();
            const uint32_t kend = nsteps - T0 < PNG_SPEC_BLOCK ? nsteps - T0 : PNG_SPEC_BLOCK;
            for (uint32_t k = 0; k < kend; k++) {
                const int g = (int)(T0 + k) - (int)lane;
                const int valid = active && g >= 0 && g < (int)ngroups;
                uint32_t U[GD + 1], V[GD + 1];
DEV_UNROLL
                for (uint32_t i = 0; i < GD; i++) U[i] = png_lane_above(R[i]);
                U[GD] = 0u;
                if (lane == 0) {
DEV_UNROLL
                    for (uint32_t i = 0; i < GD; i++) U[i] = band > 0 ? uptile[k * GD + i] : 0u;
                }
                if (valid) {
DEV_UNROLL
                    for (uint32_t i = 0; i < GD; i++) V[i] = png_funnel(tile[k * GD + i + 1u], tile[k * GD + i], row_sh);
                    V[GD] = 0u;
                    if (g == 0) {
DEV_UNROLL
                        for (uint32_t d = 0; d < ND; d++) a[d] = c[d] = 0u;
                    }
                    switch (ft) { /* per row, i.e. per lane */
                    case 0: spec_defilter_group<BPP, 0>(V, U, a, c, R); break;
                    case 1: spec_defilter_group<BPP, 1>(V, U, a, c, R); break;
                    case 2: spec_defilter_group<BPP, 2>(V, U, a, c, R); break;
                    case 3: spec_defilter_group<BPP, 3>(V, U, a, c, R); break;
                    default: spec_defilter_group<BPP, 4>(V, U, a, c, R); break;
                    }
                    if (lane == 63u) { /* the row the band below starts from */
DEV_UNROLL
                        for (uint32_t i = 0; i < GD; i++) myring[(uint32_t)g * GD + i] = R[i];
                    }
                    // ---- pixels: unpack / reduce / key / palette, strided Adam7 store
                    if constexpr (spec_out_rgba8(O())) {
                        if (BPP == 1 && depth < 8u) {
                            const uint32_t mask = (1u << depth) - 1u;
DEV_UNROLL
                            for (uint32_t j = 0; j < K; j++) {
                                const uint32_t byte = spec_get(R, j, 1u);
                                const uint64_t xb = ((uint64_t)g * K + j) * ppb;
                                for (uint32_t s = 0; s < ppb; s++) {
                                    if (xb + s >= w) break;
                                    const uint32_t smp = (byte >> (8u - depth * (s + 1u))) & mask;
                                    const uint32_t px = spec_pixel_sub(smp, ct, depth, t, L.pal, pal_bad);
                                    *reinterpret_cast<uint32_t *>(orow + (xb + s) * ostep) = px;
                                }
                            }
                        } else {
DEV_UNROLL
                            for (uint32_t j = 0; j < K; j++) {
                                const uint64_t x = (uint64_t)g * K + j;
                                if (x >= w) break;
                                const uint32_t lo = spec_get(R, j * (uint32_t)BPP, BPP < 4 ? (uint32_t)BPP : 4u);
                                const uint32_t hi = BPP > 4 ? spec_get(R, j * (uint32_t)BPP + 4u, (uint32_t)BPP - 4u) : 0u;
                                *reinterpret_cast<uint32_t *>(orow + x * ostep) = spec_pixel(lo, hi, ct, depth, t, L.pal, pal_bad);
                            }
                        }
                    } else { /* the output format of the task */
                        spec_out_group<BPP>(O(), R, g, w, depth, ct, t, L.pal, pal_bad, orow, ostep);
                    }
                }
            }
            // publish: after this block lane 63 has put the groups below T0 + kend - 63 into the ring
            wave_mem_fence();
            const int done_g = (int)(T0 + kend) - 63;
            const uint32_t g63 = done_g < 0 ? 0u : ((uint32_t)done_g > ngroups ? ngroups : (uint32_t)done_g);
            if (lane == 0) *(volatile uint32_t *)&L.progress[wv] = band * (ngroups + 1u) + g63;
        }
        if (stop) break;
    }
    if (__any(pal_bad != 0u) && lane == 0) atomicOr(&L.pal_bad, 1u);
}

template <class O>
DEV_INLINE void png_spec_tasks(PngSpecLds &L, uint8_t *__restrict__ arena, uint8_t *__restrict__ rgba_arena,
                               const debig_png_spec_task *__restrict__ tasks, debig_png_spec_result *__restrict__ results,
                               uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < n_tasks; k += gridDim.x) {
        const debig_png_spec_task t = tasks[k];
        if (t.color_type == 3u) {
            const uint32_t *pal = reinterpret_cast<const uint32_t *>(arena + t.pal_off);
            for (uint32_t i = tid; i < 256u; i += 64u * PNG_SPEC_NWD) L.pal[i] = pal[i];
        }
        if (tid < PNG_SPEC_NWD) L.progress[tid] = 0u;
        if (tid == 0) { L.first_bad = 0xffffffffu; L.pal_bad = 0u; }
        __syncthreads();
        switch (t.bpp_f) { /* workgroup-uniform */
        case 1: png_spec_task<1, O>(L, arena, rgba_arena, t, tid); break;
        case 2: png_spec_task<2, O>(L, arena, rgba_arena, t, tid); break;
        case 3: png_spec_task<3, O>(L, arena, rgba_arena, t, tid); break;
        case 4: png_spec_task<4, O>(L, arena, rgba_arena, t, tid); break;
        case 6: png_spec_task<6, O>(L, arena, rgba_arena, t, tid); break;
        case 8: png_spec_task<8, O>(L, arena, rgba_arena, t, tid); break;
        default: if (tid == 0) L.first_bad = 0xfffffffeu; break;
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t fb = L.first_bad;
            results[k].status = fb != 0xffffffffu ? DEBIG_PNG_SPEC_E_FILTER : L.pal_bad ? DEBIG_PNG_SPEC_E_PALETTE : 0u;
            results[k].bad_row = fb;
        }
        __syncthreads();
    }
}


__global__ void __launch_bounds__(64 * PNG_SPEC_NWD)
debig_png_spec_defilter_kernel(uint8_t *__restrict__ arena, uint8_t *__restrict__ rgba_arena,
                               const debig_png_spec_task *__restrict__ tasks, debig_png_spec_result *__restrict__ results,
                               uint32_t n_tasks)
{
    __shared__ PngSpecLds L;
    png_spec_tasks<PngSpecOutRgba8>(L, arena, rgba_arena, tasks, results, n_tasks);
}

// the same tasks to the output format each carries (t.out_fmt); a kernel of its own, so that the RGBA8 kernel keeps its
// registers and its occupancy
__global__ void __launch_bounds__(64 * PNG_SPEC_NWD)
debig_png_spec_defilter_fmt_kernel(uint8_t *__restrict__ arena, uint8_t *__restrict__ out_arena,
                                   const debig_png_spec_task *__restrict__ tasks, debig_png_spec_result *__restrict__ results,
                                   uint32_t n_tasks)
{
    __shared__ PngSpecLds L;
    png_spec_tasks<PngSpecOutFmt>(L, arena, out_arena, tasks, results, n_tasks);
}

// ... and to channel planes (c, y, x) instead of interleaved pixels (t.out_fmt, t.img_height): again a kernel of its own
__global__ void __launch_bounds__(64 * PNG_SPEC_NWD)
debig_png_spec_defilter_planar_kernel(uint8_t *__restrict__ arena, uint8_t *__restrict__ out_arena,
                                      const debig_png_spec_task *__restrict__ tasks, debig_png_spec_result *__restrict__ results,
                                      uint32_t n_tasks)
{
    __shared__ PngSpecLds L;
    png_spec_tasks<PngSpecOutPlanar>(L, arena, out_arena, tasks, results, n_tasks);
}

// ... and to raw labels (PngSpecOutIndex): colour types 3 and 0 only, so the body is instantiated for the filter units 1 and 2
// alone and the palette is not staged; every other task fails with the internal guard.  A kernel of its own once more: the
// kernels above keep their code, registers and occupancy.
__global__ void __launch_bounds__(64 * PNG_SPEC_NWD)
debig_png_spec_defilter_index_kernel(uint8_t *__restrict__ arena, uint8_t *__restrict__ out_arena,
                                     const debig_png_spec_task *__restrict__ tasks, debig_png_spec_result *__restrict__ results,
                                     uint32_t n_tasks)
{
    __shared__ PngSpecLds L;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < n_tasks; k += gridDim.x) {
        const debig_png_spec_task t = tasks[k];
        if (tid < PNG_SPEC_NWD) L.progress[tid] = 0u;
        if (tid == 0) { L.first_bad = 0xffffffffu; L.pal_bad = 0u; }
        __syncthreads();
        const bool label = (t.color_type == 0u || t.color_type == 3u) && t.channels == 1u; /* workgroup-uniform */
        if (label && t.bpp_f == 1u && t.depth <= 8u) png_spec_task<1, PngSpecOutIndex>(L, arena, out_arena, t, tid);
        else if (label && t.bpp_f == 2u && t.depth == 16u) png_spec_task<2, PngSpecOutIndex>(L, arena, out_arena, t, tid);
        else if (tid == 0) L.first_bad = 0xfffffffeu;
        __syncthreads();
        if (tid == 0) {
            const uint32_t fb = L.first_bad;
            results[k].status = fb != 0xffffffffu ? DEBIG_PNG_SPEC_E_FILTER : L.pal_bad ? DEBIG_PNG_SPEC_E_PALETTE : 0u;
            results[k].bad_row = fb;
        }
        __syncthreads();
    }
}
