// png_stage_common.inc -- what the tensor-stage kernels share across their files: the lane walk over the items of a row run or
// tile, the ONE conversion of a 30-bit value to an output element, the store of one label, and what the kernels that post-process
// a dense label tensor (png_label_{stats, boundary, distance, components}_kernel.inc) share: the bound tests of a task (stage_*_ok)
// and the access to an element of 1 / 2 / 4 / 8 bytes as (low word, high word) -- load, store, out of and into a 16-byte item, the
// compare, the 32-bit key, and an int64 `value` as such an element.
// (What only one family shares stays with the family's first kernel: the resize tile in png_resize_kernel.inc, the gather row
// body in png_label_kernel.inc, the colour map in png_color_label_kernel.inc, the warp picks in png_warp_kernel.inc.)
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc in front of it.

#ifdef DEBIG_EMU
#define RSZ_UNROLL
#else
#define RSZ_UNROLL _Pragma("unroll")
#endif

// items i = tid, tid + threads, ... of a run of rows of w items each, as (row r, item x of the row) without a division per
// item: the lanes run along a row, then on into the next one
struct StageWalk {
    uint32_t r, x, dr, dx, w;
    DEV_MEMBER_INLINE StageWalk(uint32_t tid, uint32_t w_, uint32_t threads)
        : r(tid / w_), x(tid - r * w_), dr(threads / w_), dx(threads - dr * w_), w(w_) {}
    __device__ __forceinline__ void next() // (forced inline in the emulator build as well, which would otherwise export it)
    {
        r += dr;
        x += dx;
        if (x >= w) { x -= w; r++; }
    }
};

// float32 bits -> float16 bits, round to nearest even (finite values that round past 65504 and infinities -> infinity)
DEV_INLINE uint32_t rsz_f16_bits(uint32_t x)
{
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u);
    if (x >= 0x477ff000u) return sign | 0x7c00u;
    if (x < 0x38800000u) { // below 2^-14: a float16 subnormal (units of 2^-24) or zero
        const uint32_t sh = 126u - (x >> 23);
        if (sh > 25u) return sign;
        const uint32_t m = (x & 0x7fffffu) | 0x800000u, half = 1u << (sh - 1u), rem = m & ((1u << sh) - 1u);
        uint32_t r = m >> sh;
        if (rem > half || (rem == half && (r & 1u))) r++;
        return sign | r;
    }
    uint32_t r = (x - 0x38000000u) >> 13;
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
    return sign | r;
}

// (float)v * a + b as two separately rounded operations (never one fused multiply-add), as float32 bits
DEV_INLINE uint32_t rsz_affine_bits(uint32_t v, float a, float b)
{
#ifndef DEBIG_EMU
#pragma clang fp contract(off)
#endif
    const float m = (float)v * a;
    const float f = m + b;
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// the ONE conversion: v30 (the sample times 2^(30 - bits)) -> one element of the output dtype (a, b: the channel's affine
// pair, float dtypes only)
DEV_INLINE void rsz_cubic_store(uint32_t dtype, uint32_t bits, float a, float b, uint8_t *o, uint64_t el, uint32_t v)
{
    if (dtype == 0u) { // DEBIG_PNG_T_UINT
        if (bits == 8u) o[el] = (uint8_t)((v + (1u << 21)) >> 22);
        else reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)((v + (1u << 13)) >> 14);
    } else {
        const uint32_t u = rsz_affine_bits(v, a, b);
        if (dtype == 1u) reinterpret_cast<uint32_t *>(o)[el] = u;                                  // F32
        else if (dtype == 2u) reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)rsz_f16_bits(u);      // F16
        else reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); // BF16
    }
}

template <uint32_t P> struct RszSample;
template <> struct RszSample<8u> { typedef uint8_t sample_t; };
template <> struct RszSample<16u> { typedef uint16_t sample_t; };

// one label of ES bytes at p (aligned to ES); int64 takes the sign of the int32
template <uint32_t ES>
DEV_INLINE void lbl_store1(uint8_t *p, uint32_t v)
{
    if (ES == 1u) {
        *p = (uint8_t)v;
    } else if (ES == 2u) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    } else if (ES == 4u) {
        *reinterpret_cast<uint32_t *>(p) = v;
    } else {
        uint2 q;
        q.x = v; q.y = (uint32_t)((int32_t)v >> 31);
        *reinterpret_cast<uint2 *>(p) = q;
    }
}

// ---- a dense label tensor as the post-processing kernels read it -------------------------------------------------------------------

// the bound tests every task of these kernels repeats: the image's sides; rows row0 .. row0 + rows - 1 inside an image of h rows;
// such a run within a budget of max_elems elements, or one row; an offset and the address base + off aligned (align_mask: the
// alignment - 1; typed loads and stores follow, and a caller's buffer need not be aligned)
DEV_INLINE bool stage_dim_ok(uint32_t w, uint32_t h) { return w != 0u && w <= 16384u && h != 0u && h <= 16384u; }
DEV_INLINE bool stage_rows_ok(uint32_t h, uint32_t row0, uint32_t rows) { return rows != 0u && row0 < h && rows <= h - row0; }
DEV_INLINE bool stage_budget_ok(uint32_t rows, uint32_t w, uint32_t max_elems) { return rows <= max_elems / w || rows == 1u; }
DEV_INLINE bool stage_addr_ok(const void *base, uint64_t off, uint64_t align_mask)
{
    return (off & align_mask) == 0u && (((uintptr_t)base + off) & align_mask) == 0u;
}

// one element of ES bytes at p (aligned to ES) as (low word, high word)
template <uint32_t ES>
DEV_INLINE uint2 lbl_load(const uint8_t *p)
{
    uint2 q;
    q.y = 0u;
    if (ES == 1u) q.x = *p;
    else if (ES == 2u) q.x = *reinterpret_cast<const uint16_t *>(p);
    else if (ES == 4u) q.x = *reinterpret_cast<const uint32_t *>(p);
    else q = *reinterpret_cast<const uint2 *>(p);
    return q;
}

template <uint32_t ES>
DEV_INLINE void lbl_store(uint8_t *p, uint2 q)
{
    if (ES == 1u) *p = (uint8_t)q.x;
    else if (ES == 2u) *reinterpret_cast<uint16_t *>(p) = (uint16_t)q.x;
    else if (ES == 4u) *reinterpret_cast<uint32_t *>(p) = q.x;
    else *reinterpret_cast<uint2 *>(p) = q;
}

// element j of the 16-byte item in w[4] as (low word, high word)
template <uint32_t ES>
DEV_INLINE uint2 lbl_item_get(const uint32_t (&w)[4], uint32_t j)
{
    uint2 q;
    q.y = 0u;
    if (ES == 1u) q.x = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
    else if (ES == 2u) q.x = (w[j >> 1] >> (16u * (j & 1u))) & 65535u;
    else if (ES == 4u) q.x = w[j];
    else { q.x = w[2u * j]; q.y = w[2u * j + 1u]; }
    return q;
}

// element j of the item in w[4] := q
template <uint32_t ES>
DEV_INLINE void lbl_item_put(uint32_t (&w)[4], uint32_t j, uint2 q)
{
    if (ES == 1u) w[j >> 2] = (w[j >> 2] & ~(255u << (8u * (j & 3u)))) | (q.x << (8u * (j & 3u)));
    else if (ES == 2u) w[j >> 1] = (w[j >> 1] & ~(65535u << (16u * (j & 1u)))) | (q.x << (16u * (j & 1u)));
    else if (ES == 4u) w[j] = q.x;
    else { w[2u * j] = q.x; w[2u * j + 1u] = q.y; }
}

// are two elements the same?  (whole: exact for packed colours and int64 ids)
DEV_INLINE bool lbl_same(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }

// an element as a 32-bit key: its value, or 0xffffffff for an int64 whose upper word is not zero
DEV_INLINE uint32_t lbl_key(uint2 q) { return q.y ? 0xffffffffu : q.x; }

// an int64 `value` as an element of ES bytes: its words -> want, and whether an element can equal it at all (uint8 and uint16 are
// zero-extended, int32 is sign-extended)
template <uint32_t ES>
DEV_INLINE bool lbl_value(int64_t value, uint2 &want)
{
    want.x = (uint32_t)(uint64_t)value;
    want.y = ES == 8u ? (uint32_t)((uint64_t)value >> 32) : 0u;
    return ES == 1u ? (value >= 0 && value <= 255) : ES == 2u ? (value >= 0 && value <= 65535)
         : ES == 4u ? (value >= -2147483647 - 1 && value <= 2147483647) : true;
}
