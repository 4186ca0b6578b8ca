// png_resize_kernel.inc -- crop + bilinear / antialiased resize + normalise of decoded PNG pixels into one dense tensor
// (include/decode_png.h: debig_png_decode_batch_tensor; include/debig_hip.h: debig_hip_png_resize_batch; + alpha, + bicubic).
//
// The arithmetic is fixed by decode_png.h: Q14 integer weights made on the host, a horizontal pass rounded to 16 bits, a
// vertical pass into 30 bits, then ONE conversion.  Every sum is an integer sum, so no result depends on its order.
//
// One TASK is a tile of tile_w x tile_h output pixels of one image; one workgroup of 256 lanes per task:
//   - the tile's slice of the horizontal weights (and each column's first tap / tap count) is staged in LDS;
//   - pass 1: item i = (source row r, column x, channel c), c fastest, lanes along i: the lanes of one row read runs of
//     `channels` adjacent samples that lie scale * channels samples apart and walk right with the tap loop, so the lines
//     of a source row are fetched from HBM once and re-read from L1; Hq goes to LDS as 16-bit at index i (lanes write
//     adjacent halfwords);
//   - pass 2: lanes along the output row -- (x, c) with c fastest when the output's channel stride is 1 (HWC: the lanes'
//     stores are adjacent elements), else x fastest inside a channel (CHW: a run of tile_w adjacent elements per plane
//     row); the tap loop walks DOWN the Hq rows, so the lanes of a wavefront read adjacent (HWC) or `channels`-strided
//     (CHW) halfwords of one LDS row: no column walk, no padding needed;
//   - the vertical weights are uniform over a row of lanes and come from memory.
// LDS: 24 KB of Hq + 8 KB of weights + 512 B of column tables = 33,280 B per workgroup.  The host sizes the tile so that
// it fits; a task that does not is skipped (never indexed out of range).  No cross-workgroup communication, no atomics.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc in front of it.

#define RSZ_THREADS 256u

struct RszLds {
    uint16_t hq[DEBIG_PNG_RESIZE_HQ_CAP];
    int16_t wx[DEBIG_PNG_RESIZE_WX_CAP];
    uint32_t fx[DEBIG_PNG_RESIZE_TILE_W], cx[DEBIG_PNG_RESIZE_TILE_W];
};

// e / ch for ch in 1..4 without a run-time division
DEV_INLINE uint32_t rsz_div_ch(uint32_t e, uint32_t ch) { return ch == 3u ? e / 3u : e >> (ch >> 1); }

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

__global__ void __launch_bounds__(RSZ_THREADS)
debig_png_resize_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                        const debig_png_resize_task *__restrict__ tasks, const uint8_t *__restrict__ weights,
                        uint32_t n_tasks)
{
    __shared__ RszLds lds;
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_resize_task t = tasks[ti];
        const uint32_t *tx = reinterpret_cast<const uint32_t *>(weights + t.wx_off);
        const uint32_t *ty = reinterpret_cast<const uint32_t *>(weights + t.wy_off);
        const uint32_t mtx = tx[0], mty = ty[0], ch = t.channels, twc = t.tile_w * ch;
        const int16_t *wxg = reinterpret_cast<const int16_t *>(tx + 2u + 2u * tx[1]);
        const int16_t *wyg = reinterpret_cast<const int16_t *>(ty + 2u + 2u * ty[1]);
        // (uniform over the workgroup: every lane skips, or none)
        if (t.tile_w == 0u || t.tile_w > DEBIG_PNG_RESIZE_TILE_W || ch == 0u || ch > 4u ||
            (uint64_t)t.tile_w * mtx > DEBIG_PNG_RESIZE_WX_CAP || (uint64_t)t.src_rows * twc > DEBIG_PNG_RESIZE_HQ_CAP)
            continue;
        __syncthreads(); // the previous task's pass 2 has read its LDS
        if (tid < t.tile_w) {
            lds.fx[tid] = tx[2u + 2u * (t.tile_x + tid)];
            lds.cx[tid] = tx[3u + 2u * (t.tile_x + tid)];
        }
        for (uint32_t i = tid; i < t.tile_w * mtx; i += RSZ_THREADS) lds.wx[i] = wxg[(uint64_t)t.tile_x * mtx + i];
        __syncthreads();
        // ---- pass 1: Hq[r][x][c] = (sum_k wx[x][k] * s[r][fx[x] + k][c] + 2^(P-3)) >> (P-2)
        const uint32_t n1 = t.src_rows * twc, sh1 = (uint32_t)t.bits - 2u, rnd1 = 1u << ((uint32_t)t.bits - 3u);
        {
            uint32_t r = tid / twc, e = tid - r * twc;
            const uint32_t dr = RSZ_THREADS / twc, de = RSZ_THREADS - dr * twc;
            for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
                const uint32_t x = rsz_div_ch(e, ch), c = e - x * ch, cnt = lds.cx[x];
                const uint64_t s0 = (uint64_t)(t.src_y0 + r) * t.src_pitch + (uint64_t)lds.fx[x] * ch + c;
                const int16_t *w = &lds.wx[x * mtx];
                uint32_t acc = 0u;
                if (t.bits == 8u) {
                    const uint8_t *p = src + t.src_off + s0;
                    for (uint32_t k = 0; k < cnt; k++) acc += (uint32_t)w[k] * p[(uint64_t)k * ch];
                } else {
                    const uint16_t *p = reinterpret_cast<const uint16_t *>(src + t.src_off) + s0;
                    for (uint32_t k = 0; k < cnt; k++) acc += (uint32_t)w[k] * p[(uint64_t)k * ch];
                }
                lds.hq[i] = (uint16_t)((acc + rnd1) >> sh1);
                r += dr;
                e += de;
                if (e >= twc) { e -= twc; r++; }
            }
        }
        __syncthreads();
        // ---- pass 2: v = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c], then the one conversion
        const uint32_t n2 = t.tile_h * twc, planar = t.out_sc != 1u;
        for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
            const uint32_t yy = i / twc, e = i - yy * twc;
            uint32_t x, c;
            if (planar) { c = e / t.tile_w; x = e - c * t.tile_w; }
            else { x = rsz_div_ch(e, ch); c = e - x * ch; }
            const uint32_t Y = t.tile_y + yy, fy = ty[2u + 2u * Y], cnt = ty[3u + 2u * Y];
            const int16_t *w = wyg + (uint64_t)Y * mty;
            const uint16_t *h = &lds.hq[(fy - t.src_y0) * twc + x * ch + c];
            uint32_t v = 0u;
            for (uint32_t k = 0; k < cnt; k++) v += (uint32_t)w[k] * h[k * twc];
            const uint64_t el = (uint64_t)(t.tile_x + x) * t.out_sx + (uint64_t)Y * t.out_sy + (uint64_t)c * t.out_sc;
            uint8_t *o = out + t.out_off;
            if (t.dtype == 0u) { // DEBIG_PNG_T_UINT
                if (t.bits == 8u) o[el] = (uint8_t)((v + (1u << 21)) >> 22);
                else reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)((v + (1u << 13)) >> 14);
            } else {
                // a[] / b[] by a select chain: a run-time index into the by-value task struct would go through scratch
                const float a = c == 0u ? t.a[0] : c == 1u ? t.a[1] : c == 2u ? t.a[2] : t.a[3];
                const float b = c == 0u ? t.b[0] : c == 1u ? t.b[1] : c == 2u ? t.b[2] : t.b[3];
                const uint32_t u = rsz_affine_bits(v, a, b);
                if (t.dtype == 1u) reinterpret_cast<uint32_t *>(o)[el] = u;                                  // F32
                else if (t.dtype == 2u) reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)rsz_f16_bits(u);      // F16
                else reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); // BF16
            }
        }
    }
}

// ---- the same with alpha: premultiply in pass 1, filter premultiplied, composite over a background in pass 2 -----------------
// (include/decode_png.h: debig_png_decode_batch_tensor_alpha; include/debig_hip.h: debig_hip_png_resize_alpha_batch).
// The source is RGBA or GRAY_ALPHA (SC = 4 or 2 interleaved samples, alpha last).  The tile, the weight tables and the LDS
// are those of the kernel above; what differs is the unit of work, a PIXEL instead of a sample:
//   - pass 1: item i = (source row r, column x), lanes along i; a tap loads the whole pixel with one naturally aligned load
//     (b16 GA8, b32 RGBA8 / GA16, b64 RGBA16), premultiplies p_c = (s_c * alpha + (M >> 1)) div M in registers (a division
//     by a constant: a multiply and a shift) and adds into SC sums; the pixel's SC Hq halfwords go to LDS as one b32 / b64 at
//     index i * SC;
//   - pass 2: item = output pixel (yy, x), lanes along x; a tap reads the pixel's SC halfwords as one b32 / b64; OVER forms
//     v'_c = v_c + (bg_c * (Vmax - v_alpha) + (M >> 1)) div M with the 32-bit identity of the header (t = q M + r) and
//     stores SC - 1 channels, PREMULTIPLIED stores all SC; a wavefront writes a run of adjacent elements per plane row (CHW)
//     or adjacent pixels of out_channels elements (HWC).
// No scratch (every per-channel array is indexed by unrolled constants), no atomics, nothing shared between workgroups.

#ifdef DEBIG_EMU
#define RSZ_UNROLL
#else
#define RSZ_UNROLL _Pragma("unroll")
#endif
#define RSZ_ALPHA_PREMULTIPLIED 1u // decode_png.h: DEBIG_PNG_ALPHA_PREMULTIPLIED
#define RSZ_ALPHA_OVER 2u          // decode_png.h: DEBIG_PNG_ALPHA_OVER

template <uint32_t P, uint32_t SC> struct RszPixel;
template <> struct RszPixel<8u, 2u> { typedef uint16_t load_t; };
template <> struct RszPixel<8u, 4u> { typedef uint32_t load_t; };
template <> struct RszPixel<16u, 2u> { typedef uint32_t load_t; };
template <> struct RszPixel<16u, 4u> { typedef uint64_t load_t; };
template <uint32_t SC> struct RszHqWord;
template <> struct RszHqWord<2u> { typedef uint32_t word_t; };
template <> struct RszHqWord<4u> { typedef uint64_t word_t; };

// one element of output channel c (a compile-time constant at every call: the selects fold away)
DEV_INLINE void rsz_alpha_store(const debig_png_resize_alpha_task &t, uint8_t *o, uint64_t el, uint32_t v, uint32_t c)
{
    if (t.dtype == 0u) { // DEBIG_PNG_T_UINT
        if (t.bits == 8u) o[el] = (uint8_t)((v + (1u << 21)) >> 22);
        else reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)((v + (1u << 13)) >> 14);
    } else {
        const float a = c == 0u ? t.a[0] : c == 1u ? t.a[1] : c == 2u ? t.a[2] : t.a[3];
        const float b = c == 0u ? t.b[0] : c == 1u ? t.b[1] : c == 2u ? t.b[2] : t.b[3];
        const uint32_t u = rsz_affine_bits(v, a, b);
        if (t.dtype == 1u) reinterpret_cast<uint32_t *>(o)[el] = u;                                  // F32
        else if (t.dtype == 2u) reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)rsz_f16_bits(u);      // F16
        else reinterpret_cast<uint16_t *>(o)[el] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); // BF16
    }
}

// the two passes of one tile for source precision P and SC source channels; the weights of the tile are in LDS already
template <uint32_t P, uint32_t SC>
DEV_INLINE void rsz_alpha_tile(RszLds &lds, const debig_png_resize_alpha_task &t, const uint8_t *__restrict__ src,
                               uint8_t *__restrict__ out, const uint32_t *ty, const int16_t *wyg, uint32_t mtx, uint32_t mty,
                               uint32_t tid)
{
    typedef typename RszPixel<P, SC>::load_t load_t;
    typedef typename RszHqWord<SC>::word_t word_t;
    constexpr uint32_t M = (1u << P) - 1u, HALF = M >> 1, S = 30u - P, VMAX = M << S;
    const uint32_t tw = t.tile_w;
    word_t *hqw = reinterpret_cast<word_t *>(lds.hq);
    // ---- pass 1: Hq[r][x][c] = (sum_k wx[x][k] * p[r][fx[x] + k][c] + 2^(P-3)) >> (P-2), p premultiplied
    {
        const uint32_t n1 = t.src_rows * tw;
        uint32_t r = tid / tw, x = tid - r * tw;
        const uint32_t dr = RSZ_THREADS / tw, dx = RSZ_THREADS - dr * tw;
        for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
            const uint32_t cnt = lds.cx[x];
            const int16_t *w = &lds.wx[x * mtx];
            const load_t *p = reinterpret_cast<const load_t *>(src + t.src_off + (uint64_t)(t.src_y0 + r) * t.src_pitch * (P / 8u)) + lds.fx[x];
            uint32_t acc[SC];
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) acc[c] = 0u;
            for (uint32_t k = 0; k < cnt; k++) {
                const load_t px = p[k];
                const uint32_t wk = (uint32_t)w[k], al = (uint32_t)(px >> ((SC - 1u) * P)) & M;
RSZ_UNROLL
                for (uint32_t c = 0; c + 1u < SC; c++) acc[c] += wk * ((((uint32_t)(px >> (c * P)) & M) * al + HALF) / M);
                acc[SC - 1u] += wk * al;
            }
            word_t h = 0;
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) h |= (word_t)((acc[c] + (1u << (P - 3u))) >> (P - 2u)) << (16u * c);
            hqw[i] = h;
            r += dr;
            x += dx;
            if (x >= tw) { x -= tw; r++; }
        }
    }
    __syncthreads();
    // ---- pass 2: v_c = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c]; OVER adds the background's share; the one conversion
    const uint32_t n2 = t.tile_h * tw, over = t.mode == RSZ_ALPHA_OVER;
    for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
        const uint32_t yy = i / tw, x = i - yy * tw;
        const uint32_t Y = t.tile_y + yy, fy = ty[2u + 2u * Y], cnt = ty[3u + 2u * Y];
        const int16_t *w = wyg + (uint64_t)Y * mty;
        const word_t *h = &hqw[(fy - t.src_y0) * tw + x];
        uint32_t v[SC];
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++) v[c] = 0u;
        for (uint32_t k = 0; k < cnt; k++) {
            const word_t hk = h[k * tw];
            const uint32_t wk = (uint32_t)w[k];
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) v[c] += wk * ((uint32_t)(hk >> (16u * c)) & 0xffffu);
        }
        const uint64_t el = (uint64_t)(t.tile_x + x) * t.out_sx + (uint64_t)Y * t.out_sy;
        uint8_t *o = out + t.out_off;
        if (over) {
            const uint32_t tr = VMAX - v[SC - 1u], q = tr / M, rm = tr - q * M; // v_alpha <= Vmax (weights >= 0, sum 2^14)
RSZ_UNROLL
            for (uint32_t c = 0; c + 1u < SC; c++) {
                const uint32_t b = t.bg[c];
                rsz_alpha_store(t, o, el + (uint64_t)c * t.out_sc, v[c] + b * q + (b * rm + HALF) / M, c);
            }
        } else {
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) rsz_alpha_store(t, o, el + (uint64_t)c * t.out_sc, v[c], c);
        }
    }
}

__global__ void __launch_bounds__(RSZ_THREADS)
debig_png_resize_alpha_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                              const debig_png_resize_alpha_task *__restrict__ tasks, const uint8_t *__restrict__ weights,
                              uint32_t n_tasks)
{
    __shared__ __attribute__((aligned(16))) RszLds lds;
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_resize_alpha_task t = tasks[ti];
        const uint32_t *tx = reinterpret_cast<const uint32_t *>(weights + t.wx_off);
        const uint32_t *ty = reinterpret_cast<const uint32_t *>(weights + t.wy_off);
        const uint32_t mtx = tx[0], mty = ty[0], sc = t.channels;
        const int16_t *wxg = reinterpret_cast<const int16_t *>(tx + 2u + 2u * tx[1]);
        const int16_t *wyg = reinterpret_cast<const int16_t *>(ty + 2u + 2u * ty[1]);
        // (uniform over the workgroup: every lane skips, or none)
        if (t.tile_w == 0u || t.tile_w > DEBIG_PNG_RESIZE_TILE_W || (sc != 2u && sc != 4u) || t.src_channels != sc ||
            (t.bits != 8u && t.bits != 16u) || t.dtype > 3u ||
            !((t.mode == RSZ_ALPHA_OVER && t.out_channels == sc - 1u) || (t.mode == RSZ_ALPHA_PREMULTIPLIED && t.out_channels == sc)) ||
            (uint64_t)t.tile_w * mtx > DEBIG_PNG_RESIZE_WX_CAP || (uint64_t)t.src_rows * t.tile_w * sc > DEBIG_PNG_RESIZE_HQ_CAP)
            continue;
        __syncthreads(); // the previous task's pass 2 has read its LDS
        if (tid < t.tile_w) {
            lds.fx[tid] = tx[2u + 2u * (t.tile_x + tid)];
            lds.cx[tid] = tx[3u + 2u * (t.tile_x + tid)];
        }
        for (uint32_t i = tid; i < t.tile_w * mtx; i += RSZ_THREADS) lds.wx[i] = wxg[(uint64_t)t.tile_x * mtx + i];
        __syncthreads();
        if (t.bits == 8u) {
            if (sc == 4u) rsz_alpha_tile<8u, 4u>(lds, t, src, out, ty, wyg, mtx, mty, tid);
            else rsz_alpha_tile<8u, 2u>(lds, t, src, out, ty, wyg, mtx, mty, tid);
        } else {
            if (sc == 4u) rsz_alpha_tile<16u, 4u>(lds, t, src, out, ty, wyg, mtx, mty, tid);
            else rsz_alpha_tile<16u, 2u>(lds, t, src, out, ty, wyg, mtx, mty, tid);
        }
    }
}

// ---- the signed filter: bicubic (weights of either sign), straight or with alpha ---------------------------------------------
// (include/decode_png.h: debig_png_decode_batch_tensor_filter; include/debig_hip.h: debig_hip_png_resize_cubic_batch).
// The tile, the weight tables and the LDS are those of the kernels above.  What differs is the arithmetic, fixed by
// decode_png.h: signed 32-bit sums, the intermediate Hq = clamp(((h + 2^(P-2)) >> (P-1)) + 16384, 0, 65535) -- the sample at
// scale 2^15, biased by a quarter of the 16-bit range so that overshoot on either side survives pass 1 --, the bias leaving
// pass 2 as the one constant 2^28 (the vertical weights sum to exactly 2^14), then v30 = clamp(v, 0, M << (29 - P)) << 1 and
// the ONE conversion of the kernels above.  With alpha: v30_alpha is clamped first, every colour then to [0, v30_alpha].
//   - 2 and 4 source channels, every mode: the PIXEL mapping of the alpha kernel (one naturally aligned load per tap, one
//     b32 / b64 of LDS per pixel, lanes along x in pass 2); STRAIGHT skips the premultiply and clamps every channel alone;
//   - 1 and 3 source channels (STRAIGHT only): the SAMPLE mapping of the plain kernel.
// t is the task by value (uniform fields); the per-channel a[] / b[] / bg[] are read through tg, the task in global memory,
// where a run-time channel index costs nothing (into the by-value struct it would go through scratch).
// No scratch (every per-channel register array is indexed by unrolled constants), no atomics, nothing shared between workgroups.

#define RSZ_ALPHA_STRAIGHT 0u // decode_png.h: DEBIG_PNG_ALPHA_STRAIGHT
#define RSZ_CUBIC_BIAS 16384

DEV_INLINE uint32_t rsz_cubic_hq(int32_t h, uint32_t P)
{
    const int32_t q = ((h + (int32_t)(1u << (P - 2u))) >> (P - 1u)) + RSZ_CUBIC_BIAS;
    return (uint32_t)(q < 0 ? 0 : q > 65535 ? 65535 : q);
}

// v (the sample times 2^(29 - P), signed) -> v30 inside [0, Vmax]
DEV_INLINE uint32_t rsz_cubic_v30(int32_t v, uint32_t P)
{
    const int32_t top = (int32_t)(((1u << P) - 1u) << (29u - P));
    return (uint32_t)(v < 0 ? 0 : v > top ? top : v) << 1;
}

// one element: v30 -> the output dtype (a, b: the channel's affine pair, float dtypes only)
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

// pass 1 of the pixel mapping: Hq[r][x][c] of the tile's source rows; PM: premultiply as the pixel is read
template <uint32_t P, uint32_t SC, bool PM>
DEV_INLINE void rsz_cubic_pixel_pass1(RszLds &lds, const debig_png_resize_cubic_task &t, const uint8_t *__restrict__ src,
                                      uint32_t mtx, uint32_t tid)
{
    typedef typename RszPixel<P, SC>::load_t load_t;
    typedef typename RszHqWord<SC>::word_t word_t;
    constexpr uint32_t M = (1u << P) - 1u, HALF = M >> 1;
    const uint32_t tw = t.tile_w, n1 = t.src_rows * tw;
    word_t *hqw = reinterpret_cast<word_t *>(lds.hq);
    uint32_t r = tid / tw, x = tid - r * tw;
    const uint32_t dr = RSZ_THREADS / tw, dx = RSZ_THREADS - dr * tw;
    for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
        const uint32_t cnt = lds.cx[x];
        const int16_t *w = &lds.wx[x * mtx];
        const load_t *p = reinterpret_cast<const load_t *>(src + t.src_off + (uint64_t)(t.src_y0 + r) * t.src_pitch * (P / 8u)) + lds.fx[x];
        int32_t acc[SC];
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++) acc[c] = 0;
        for (uint32_t k = 0; k < cnt; k++) {
            const load_t px = p[k];
            const int32_t wk = w[k];
            const uint32_t al = (uint32_t)(px >> ((SC - 1u) * P)) & M;
RSZ_UNROLL
            for (uint32_t c = 0; c + 1u < SC; c++) {
                const uint32_t s = (uint32_t)(px >> (c * P)) & M;
                acc[c] += wk * (int32_t)(PM ? (s * al + HALF) / M : s);
            }
            acc[SC - 1u] += wk * (int32_t)al;
        }
        word_t h = 0;
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++) h |= (word_t)rsz_cubic_hq(acc[c], P) << (16u * c);
        hqw[i] = h;
        r += dr;
        x += dx;
        if (x >= tw) { x -= tw; r++; }
    }
}

// the two passes of one tile at the pixel mapping, for source precision P and SC = 2 or 4 source channels
template <uint32_t P, uint32_t SC>
DEV_INLINE void rsz_cubic_pixel_tile(RszLds &lds, const debig_png_resize_cubic_task &t,
                                     const debig_png_resize_cubic_task *__restrict__ tg, const uint8_t *__restrict__ src,
                                     uint8_t *__restrict__ out, const uint32_t *ty, const int16_t *wyg, uint32_t mtx, uint32_t mty,
                                     uint32_t tid)
{
    typedef typename RszHqWord<SC>::word_t word_t;
    constexpr uint32_t M = (1u << P) - 1u, HALF = M >> 1, S = 30u - P, VMAX = M << S;
    const uint32_t tw = t.tile_w;
    const word_t *hqw = reinterpret_cast<const word_t *>(lds.hq);
    if (t.mode == RSZ_ALPHA_STRAIGHT) rsz_cubic_pixel_pass1<P, SC, false>(lds, t, src, mtx, tid);
    else rsz_cubic_pixel_pass1<P, SC, true>(lds, t, src, mtx, tid);
    __syncthreads();
    // ---- pass 2: v_c = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c] - 2^28; the clamps; OVER adds the background's share
    const uint32_t n2 = t.tile_h * tw;
    for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
        const uint32_t yy = i / tw, x = i - yy * tw;
        const uint32_t Y = t.tile_y + yy, fy = ty[2u + 2u * Y], cnt = ty[3u + 2u * Y];
        const int16_t *w = wyg + (uint64_t)Y * mty;
        const word_t *h = &hqw[(fy - t.src_y0) * tw + x];
        int32_t acc[SC];
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++) acc[c] = -(RSZ_CUBIC_BIAS << 14);
        for (uint32_t k = 0; k < cnt; k++) {
            const word_t hk = h[k * tw];
            const int32_t wk = w[k];
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) acc[c] += wk * (int32_t)((uint32_t)(hk >> (16u * c)) & 0xffffu);
        }
        uint32_t v[SC];
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++) v[c] = rsz_cubic_v30(acc[c], P);
        const uint64_t el = (uint64_t)(t.tile_x + x) * t.out_sx + (uint64_t)Y * t.out_sy;
        uint8_t *o = out + t.out_off;
        if (t.mode == RSZ_ALPHA_STRAIGHT) {
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, v[c]);
            continue;
        }
RSZ_UNROLL
        for (uint32_t c = 0; c + 1u < SC; c++) v[c] = v[c] < v[SC - 1u] ? v[c] : v[SC - 1u]; // with negative lobes v_c <= v_alpha must be made
        if (t.mode == RSZ_ALPHA_OVER) {
            const uint32_t tr = VMAX - v[SC - 1u], q = tr / M, rm = tr - q * M;
RSZ_UNROLL
            for (uint32_t c = 0; c + 1u < SC; c++) {
                const uint32_t b = tg->bg[c];
                rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, v[c] + b * q + (b * rm + HALF) / M);
            }
        } else {
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, v[c]);
        }
    }
}

// the two passes of one tile at the sample mapping (1 or 3 channels, STRAIGHT), for source precision P
template <uint32_t P>
DEV_INLINE void rsz_cubic_sample_tile(RszLds &lds, const debig_png_resize_cubic_task &t,
                                      const debig_png_resize_cubic_task *__restrict__ tg, const uint8_t *__restrict__ src,
                                      uint8_t *__restrict__ out, const uint32_t *ty, const int16_t *wyg, uint32_t mtx, uint32_t mty,
                                      uint32_t tid)
{
    typedef typename RszSample<P>::sample_t sample_t;
    const uint32_t ch = t.channels, twc = t.tile_w * ch;
    // ---- pass 1: item (source row r, column x, channel c), c fastest
    {
        const uint32_t n1 = t.src_rows * twc;
        uint32_t r = tid / twc, e = tid - r * twc;
        const uint32_t dr = RSZ_THREADS / twc, de = RSZ_THREADS - dr * twc;
        for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
            const uint32_t x = rsz_div_ch(e, ch), c = e - x * ch, cnt = lds.cx[x];
            const int16_t *w = &lds.wx[x * mtx];
            const sample_t *p = reinterpret_cast<const sample_t *>(src + t.src_off) + (uint64_t)(t.src_y0 + r) * t.src_pitch +
                                (uint64_t)lds.fx[x] * ch + c;
            int32_t acc = 0;
            for (uint32_t k = 0; k < cnt; k++) acc += (int32_t)w[k] * (int32_t)p[(uint64_t)k * ch];
            lds.hq[i] = (uint16_t)rsz_cubic_hq(acc, P);
            r += dr;
            e += de;
            if (e >= twc) { e -= twc; r++; }
        }
    }
    __syncthreads();
    // ---- pass 2: lanes along the output row ((x, c) for HWC, x inside a channel for CHW)
    const uint32_t n2 = t.tile_h * twc, planar = t.out_sc != 1u;
    for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
        const uint32_t yy = i / twc, e = i - yy * twc;
        uint32_t x, c;
        if (planar) { c = e / t.tile_w; x = e - c * t.tile_w; }
        else { x = rsz_div_ch(e, ch); c = e - x * ch; }
        const uint32_t Y = t.tile_y + yy, fy = ty[2u + 2u * Y], cnt = ty[3u + 2u * Y];
        const int16_t *w = wyg + (uint64_t)Y * mty;
        const uint16_t *h = &lds.hq[(fy - t.src_y0) * twc + x * ch + c];
        int32_t acc = -(RSZ_CUBIC_BIAS << 14);
        for (uint32_t k = 0; k < cnt; k++) acc += (int32_t)w[k] * (int32_t)h[k * twc];
        const uint64_t el = (uint64_t)(t.tile_x + x) * t.out_sx + (uint64_t)Y * t.out_sy + (uint64_t)c * t.out_sc;
        rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], out + t.out_off, el, rsz_cubic_v30(acc, P));
    }
}

__global__ void __launch_bounds__(RSZ_THREADS)
debig_png_resize_cubic_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                              const debig_png_resize_cubic_task *__restrict__ tasks, const uint8_t *__restrict__ weights,
                              uint32_t n_tasks)
{
    __shared__ __attribute__((aligned(16))) RszLds lds;
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_resize_cubic_task t = tasks[ti];
        const uint32_t *tx = reinterpret_cast<const uint32_t *>(weights + t.wx_off);
        const uint32_t *ty = reinterpret_cast<const uint32_t *>(weights + t.wy_off);
        const uint32_t mtx = tx[0], mty = ty[0], sc = t.channels;
        const int16_t *wxg = reinterpret_cast<const int16_t *>(tx + 2u + 2u * tx[1]);
        const int16_t *wyg = reinterpret_cast<const int16_t *>(ty + 2u + 2u * ty[1]);
        const bool pixel = sc == 2u || sc == 4u;
        // (uniform over the workgroup: every lane skips, or none)
        if (t.tile_w == 0u || t.tile_w > DEBIG_PNG_RESIZE_TILE_W || sc == 0u || sc > 4u || t.src_channels != sc ||
            (t.bits != 8u && t.bits != 16u) || t.dtype > 3u ||
            !((t.mode == RSZ_ALPHA_STRAIGHT && t.out_channels == sc) || (pixel && t.mode == RSZ_ALPHA_OVER && t.out_channels == sc - 1u) ||
              (pixel && t.mode == RSZ_ALPHA_PREMULTIPLIED && t.out_channels == sc)) ||
            (uint64_t)t.tile_w * mtx > DEBIG_PNG_RESIZE_WX_CAP || (uint64_t)t.src_rows * t.tile_w * sc > DEBIG_PNG_RESIZE_HQ_CAP)
            continue;
        __syncthreads(); // the previous task's pass 2 has read its LDS
        if (tid < t.tile_w) {
            lds.fx[tid] = tx[2u + 2u * (t.tile_x + tid)];
            lds.cx[tid] = tx[3u + 2u * (t.tile_x + tid)];
        }
        for (uint32_t i = tid; i < t.tile_w * mtx; i += RSZ_THREADS) lds.wx[i] = wxg[(uint64_t)t.tile_x * mtx + i];
        __syncthreads();
        if (t.bits == 8u) {
            if (sc == 4u) rsz_cubic_pixel_tile<8u, 4u>(lds, t, &tasks[ti], src, out, ty, wyg, mtx, mty, tid);
            else if (sc == 2u) rsz_cubic_pixel_tile<8u, 2u>(lds, t, &tasks[ti], src, out, ty, wyg, mtx, mty, tid);
            else rsz_cubic_sample_tile<8u>(lds, t, &tasks[ti], src, out, ty, wyg, mtx, mty, tid);
        } else {
            if (sc == 4u) rsz_cubic_pixel_tile<16u, 4u>(lds, t, &tasks[ti], src, out, ty, wyg, mtx, mty, tid);
            else if (sc == 2u) rsz_cubic_pixel_tile<16u, 2u>(lds, t, &tasks[ti], src, out, ty, wyg, mtx, mty, tid);
            else rsz_cubic_sample_tile<16u>(lds, t, &tasks[ti], src, out, ty, wyg, mtx, mty, tid);
        }
    }
}
