// png_stage_common.inc -- what the tensor-stage kernels share across their files: the lane walk over the items of a row run or
// tile, the ONE conversion of a 30-bit value to an output element, and the store of one label.
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
