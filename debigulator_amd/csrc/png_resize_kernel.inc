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
// The top of a tile (rsz_tile_begin) and the two pass-1 bodies (rsz_sample_pass1, rsz_pixel_pass1) exist once, for the
// kernels of the family and for debig_png_resize_color_kernel (png_color_kernel.inc) -- but for the bicubic kernel, which
// states the top of its tile itself (its comment says why); the conversion is rsz_cubic_store.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_stage_common.inc in front of it.

#define RSZ_THREADS 256u

struct RszLds {
    uint16_t hq[DEBIG_PNG_RESIZE_HQ_CAP];
    int16_t wx[DEBIG_PNG_RESIZE_WX_CAP];
    uint32_t fx[DEBIG_PNG_RESIZE_TILE_W], cx[DEBIG_PNG_RESIZE_TILE_W];
};

// e / ch for ch in 1..4 without a run-time division
DEV_INLINE uint32_t rsz_div_ch(uint32_t e, uint32_t ch) { return ch == 3u ? e / 3u : e >> (ch >> 1); }

// what the top of a tile leaves for pass 2: the vertical axis table, its weights, the tap capacities of both axes
struct RszAxes {
    const uint32_t *ty;
    const int16_t *wyg;
    uint32_t mtx, mty;
};

// the top of a tile, shared by the kernels of the family: the axis tables of the task, the tile bounds (on t.channels, the
// SOURCE channel count), then the tile's slice of the horizontal table into LDS between two barriers.  false: the task breaks
// a bound and is skipped.  Everything tested is uniform over the workgroup -- every lane skips, or none -- and the skip comes
// before the first barrier.  A kernel tests the fields only it knows before it calls this; more() is for a test that has to
// come behind the shared ones and must still skip before the barrier (the colour kernel reads its record there, as uniform as
// the rest).
template <class Task, class More>
DEV_INLINE bool rsz_tile_begin(RszLds &lds, const Task &t, const uint8_t *__restrict__ weights, uint32_t tid, RszAxes &ax, More more)
{
    const uint32_t *tx = reinterpret_cast<const uint32_t *>(weights + t.wx_off);
    const uint32_t *ty = reinterpret_cast<const uint32_t *>(weights + t.wy_off);
    const uint32_t mtx = tx[0], ch = t.channels;
    const int16_t *wxg = reinterpret_cast<const int16_t *>(tx + 2u + 2u * tx[1]);
    ax.ty = ty;
    ax.wyg = reinterpret_cast<const int16_t *>(ty + 2u + 2u * ty[1]);
    ax.mtx = mtx;
    ax.mty = ty[0];
    if (t.tile_w == 0u || t.tile_w > DEBIG_PNG_RESIZE_TILE_W || ch == 0u || ch > 4u ||
        (uint64_t)t.tile_w * mtx > DEBIG_PNG_RESIZE_WX_CAP || (uint64_t)t.src_rows * (t.tile_w * ch) > DEBIG_PNG_RESIZE_HQ_CAP)
        return false;
    if (!more()) return false;
    __syncthreads(); // the previous task's pass 2 has read its LDS
    if (tid < t.tile_w) {
        lds.fx[tid] = tx[2u + 2u * (t.tile_x + tid)];
        lds.cx[tid] = tx[3u + 2u * (t.tile_x + tid)];
    }
    for (uint32_t i = tid; i < t.tile_w * mtx; i += RSZ_THREADS) lds.wx[i] = wxg[(uint64_t)t.tile_x * mtx + i];
    __syncthreads();
    return true;
}
template <class Task>
DEV_INLINE bool rsz_tile_begin(RszLds &lds, const Task &t, const uint8_t *__restrict__ weights, uint32_t tid, RszAxes &ax)
{
    return rsz_tile_begin(lds, t, weights, tid, ax, [] { return true; });
}

// pass 1 of the sample mapping, unsigned weights, the precision a run-time value:
// Hq[r][x][c] = (sum_k wx[x][k] * s[r][fx[x] + k][c] + 2^(P-3)) >> (P-2)
template <class Task>
DEV_INLINE void rsz_sample_pass1(RszLds &lds, const Task &t, const uint8_t *__restrict__ src, uint32_t mtx, uint32_t tid)
{
    const uint32_t ch = t.channels, twc = t.tile_w * ch;
    const uint32_t n1 = t.src_rows * twc, sh1 = (uint32_t)t.bits - 2u, rnd1 = 1u << ((uint32_t)t.bits - 3u);
    StageWalk wk(tid, twc, RSZ_THREADS);
    for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
        const uint32_t x = rsz_div_ch(wk.x, ch), c = wk.x - x * ch, cnt = lds.cx[x];
        const uint64_t s0 = (uint64_t)(t.src_y0 + wk.r) * t.src_pitch + (uint64_t)lds.fx[x] * ch + c;
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
        wk.next();
    }
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
        RszAxes ax;
        if (!rsz_tile_begin(lds, t, weights, tid, ax)) continue;
        rsz_sample_pass1(lds, t, src, ax.mtx, tid);
        __syncthreads();
        // ---- pass 2: v = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c], then the one conversion
        const uint32_t ch = t.channels, twc = t.tile_w * ch, n2 = t.tile_h * twc, planar = t.out_sc != 1u;
        for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
            const uint32_t yy = i / twc, e = i - yy * twc;
            uint32_t x, c;
            if (planar) { c = e / t.tile_w; x = e - c * t.tile_w; }
            else { x = rsz_div_ch(e, ch); c = e - x * ch; }
            const uint32_t Y = t.tile_y + yy, fy = ax.ty[2u + 2u * Y], cnt = ax.ty[3u + 2u * Y];
            const int16_t *w = ax.wyg + (uint64_t)Y * ax.mty;
            const uint16_t *h = &lds.hq[(fy - t.src_y0) * twc + x * ch + c];
            uint32_t v = 0u;
            for (uint32_t k = 0; k < cnt; k++) v += (uint32_t)w[k] * h[k * twc];
            const uint64_t el = (uint64_t)(t.tile_x + x) * t.out_sx + (uint64_t)Y * t.out_sy + (uint64_t)c * t.out_sc;
            // a[] / b[] by a select chain: a run-time index into the by-value task struct would go through scratch
            const float a = c == 0u ? t.a[0] : c == 1u ? t.a[1] : c == 2u ? t.a[2] : t.a[3];
            const float b = c == 0u ? t.b[0] : c == 1u ? t.b[1] : c == 2u ? t.b[2] : t.b[3];
            rsz_cubic_store(t.dtype, t.bits, a, b, out + t.out_off, el, v);
        }
    }
}

// ---- the same with alpha: premultiply in pass 1, filter premultiplied, composite over a background in pass 2 -----------------
// (include/decode_png.h: debig_png_decode_batch_tensor_alpha; include/debig_hip.h: debig_hip_png_resize_alpha_batch).
// The source is RGBA or GRAY_ALPHA (SC = 4 or 2 interleaved samples, alpha last).  The tile, the weight tables and the LDS
// are those of the kernel above (rsz_tile_begin); what differs is the unit of work, a PIXEL instead of a sample
// (rsz_pixel_pass1):
//   - pass 1: item i = (source row r, column x), lanes along i; a tap loads the whole pixel with one naturally aligned load
//     (b16 GA8, b32 RGBA8 / GA16, b64 RGBA16), premultiplies p_c = (s_c * alpha + (M >> 1)) div M in registers (a division
//     by a constant: a multiply and a shift) and adds into SC sums; the pixel's SC Hq halfwords go to LDS as one b32 / b64 at
//     index i * SC;
//   - pass 2: item = output pixel (yy, x), lanes along x; a tap reads the pixel's SC halfwords as one b32 / b64; OVER forms
//     v'_c = v_c + (bg_c * (Vmax - v_alpha) + (M >> 1)) div M with the 32-bit identity of the header (t = q M + r) and
//     stores SC - 1 channels, PREMULTIPLIED stores all SC; a wavefront writes a run of adjacent elements per plane row (CHW)
//     or adjacent pixels of out_channels elements (HWC).
// No scratch (every per-channel array is indexed by unrolled constants), no atomics, nothing shared between workgroups.

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
template <bool SG> struct RszSum; // the 32-bit sums of pass 1: unsigned weights, or the signed filter's
template <> struct RszSum<false> { typedef uint32_t sum_t; };
template <> struct RszSum<true> { typedef int32_t sum_t; };

// the signed filter's intermediate (the bicubic section below has the rule): the sample at scale 2^15, biased and clamped
#define RSZ_CUBIC_BIAS 16384
DEV_INLINE uint32_t rsz_cubic_hq(int32_t h, uint32_t P)
{
    const int32_t q = ((h + (int32_t)(1u << (P - 2u))) >> (P - 1u)) + RSZ_CUBIC_BIAS;
    return (uint32_t)(q < 0 ? 0 : q > 65535 ? 65535 : q);
}

// pass 1 of the pixel mapping, for source precision P and SC source channels: Hq[r][x][c] of the tile's source rows, the
// pixel's SC halfwords as one word.  PM: premultiply as the pixel is read; SG: the signed filter -- signed sums and its Hq
// (rsz_cubic_hq) instead of (sum + 2^(P-3)) >> (P-2).
template <uint32_t P, uint32_t SC, bool PM, bool SG, class Task>
DEV_INLINE void rsz_pixel_pass1(RszLds &lds, const Task &t, const uint8_t *__restrict__ src, uint32_t mtx, uint32_t tid)
{
    typedef typename RszPixel<P, SC>::load_t load_t;
    typedef typename RszHqWord<SC>::word_t word_t;
    typedef typename RszSum<SG>::sum_t sum_t;
    constexpr uint32_t M = (1u << P) - 1u, HALF = M >> 1;
    const uint32_t n1 = t.src_rows * t.tile_w;
    word_t *hqw = reinterpret_cast<word_t *>(lds.hq);
    StageWalk wk(tid, t.tile_w, RSZ_THREADS);
    for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
        const uint32_t cnt = lds.cx[wk.x];
        const int16_t *w = &lds.wx[wk.x * mtx];
        const load_t *p = reinterpret_cast<const load_t *>(src + t.src_off + (uint64_t)(t.src_y0 + wk.r) * t.src_pitch * (P / 8u)) + lds.fx[wk.x];
        sum_t acc[SC];
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++) acc[c] = 0;
        for (uint32_t k = 0; k < cnt; k++) {
            const load_t px = p[k];
            const sum_t wgt = (sum_t)w[k];
            const uint32_t al = (uint32_t)(px >> ((SC - 1u) * P)) & M;
RSZ_UNROLL
            for (uint32_t c = 0; c + 1u < SC; c++) {
                const uint32_t s = (uint32_t)(px >> (c * P)) & M;
                acc[c] += wgt * (sum_t)(PM ? (s * al + HALF) / M : s);
            }
            acc[SC - 1u] += wgt * (sum_t)al;
        }
        word_t h = 0;
RSZ_UNROLL
        for (uint32_t c = 0; c < SC; c++)
            h |= (word_t)(SG ? rsz_cubic_hq((int32_t)acc[c], P) : ((uint32_t)acc[c] + (1u << (P - 3u))) >> (P - 2u)) << (16u * c);
        hqw[i] = h;
        wk.next();
    }
}

// the two passes of one tile for source precision P and SC source channels; the weights of the tile are in LDS already
template <uint32_t P, uint32_t SC>
DEV_INLINE void rsz_alpha_tile(RszLds &lds, const debig_png_resize_alpha_task &t, const uint8_t *__restrict__ src,
                               uint8_t *__restrict__ out, const RszAxes &ax, uint32_t tid)
{
    typedef typename RszHqWord<SC>::word_t word_t;
    constexpr uint32_t M = (1u << P) - 1u, HALF = M >> 1, S = 30u - P, VMAX = M << S;
    const uint32_t tw = t.tile_w;
    const word_t *hqw = reinterpret_cast<const word_t *>(lds.hq);
    rsz_pixel_pass1<P, SC, true, false>(lds, t, src, ax.mtx, tid);
    __syncthreads();
    // ---- pass 2: v_c = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c]; OVER adds the background's share; the one conversion
    const uint32_t n2 = t.tile_h * tw, over = t.mode == RSZ_ALPHA_OVER;
    for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
        const uint32_t yy = i / tw, x = i - yy * tw;
        const uint32_t Y = t.tile_y + yy, fy = ax.ty[2u + 2u * Y], cnt = ax.ty[3u + 2u * Y];
        const int16_t *w = ax.wyg + (uint64_t)Y * ax.mty;
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
        // (c is a compile-time constant at every store: a[c] / b[c] / bg[c] of the by-value task stay in registers)
        if (over) {
            const uint32_t tr = VMAX - v[SC - 1u], q = tr / M, rm = tr - q * M; // v_alpha <= Vmax (weights >= 0, sum 2^14)
RSZ_UNROLL
            for (uint32_t c = 0; c + 1u < SC; c++) {
                const uint32_t b = t.bg[c];
                rsz_cubic_store(t.dtype, P, t.a[c], t.b[c], o, el + (uint64_t)c * t.out_sc, v[c] + b * q + (b * rm + HALF) / M);
            }
        } else {
RSZ_UNROLL
            for (uint32_t c = 0; c < SC; c++) rsz_cubic_store(t.dtype, P, t.a[c], t.b[c], o, el + (uint64_t)c * t.out_sc, v[c]);
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
        const uint32_t sc = t.channels;
        RszAxes ax;
        // (uniform over the workgroup: every lane skips, or none)
        if ((sc != 2u && sc != 4u) || t.src_channels != sc || (t.bits != 8u && t.bits != 16u) || t.dtype > 3u ||
            !((t.mode == RSZ_ALPHA_OVER && t.out_channels == sc - 1u) || (t.mode == RSZ_ALPHA_PREMULTIPLIED && t.out_channels == sc)))
            continue;
        if (!rsz_tile_begin(lds, t, weights, tid, ax)) continue;
        if (t.bits == 8u) {
            if (sc == 4u) rsz_alpha_tile<8u, 4u>(lds, t, src, out, ax, tid);
            else rsz_alpha_tile<8u, 2u>(lds, t, src, out, ax, tid);
        } else {
            if (sc == 4u) rsz_alpha_tile<16u, 4u>(lds, t, src, out, ax, tid);
            else rsz_alpha_tile<16u, 2u>(lds, t, src, out, ax, tid);
        }
    }
}

// ---- the signed filter: bicubic (weights of either sign), straight or with alpha ---------------------------------------------
// (include/decode_png.h: debig_png_decode_batch_tensor_filter; include/debig_hip.h: debig_hip_png_resize_cubic_batch).
// The tile, the weight tables and the LDS are those of the kernels above (rsz_tile_begin).  What differs is the arithmetic, fixed by
// decode_png.h: signed 32-bit sums, the intermediate Hq = clamp(((h + 2^(P-2)) >> (P-1)) + 16384, 0, 65535) -- the sample at
// scale 2^15, biased by a quarter of the 16-bit range so that overshoot on either side survives pass 1 --, the bias leaving
// pass 2 as the one constant 2^28 (the vertical weights sum to exactly 2^14), then v30 = clamp(v, 0, M << (29 - P)) << 1 and
// the ONE conversion of the kernels above.  With alpha: v30_alpha is clamped first, every colour then to [0, v30_alpha].
//   - 2 and 4 source channels, every mode: the PIXEL mapping of the alpha kernel (rsz_pixel_pass1 with the signed Hq: one
//     naturally aligned load per tap, one b32 / b64 of LDS per pixel, lanes along x in pass 2); STRAIGHT skips the premultiply
//     and clamps every channel alone;
//   - 1 and 3 source channels (STRAIGHT only): the SAMPLE mapping of the plain kernel, with a pass 1 of its own (signed sums
//     at a compile-time P, where rsz_sample_pass1 is unsigned at a run-time one).
// t is the task by value (uniform fields); the per-channel a[] / b[] / bg[] are read through tg, the task in global memory,
// where a run-time channel index costs nothing (into the by-value struct it would go through scratch).
// No scratch (every per-channel register array is indexed by unrolled constants), no atomics, nothing shared between workgroups.

#define RSZ_ALPHA_STRAIGHT 0u // decode_png.h: DEBIG_PNG_ALPHA_STRAIGHT

// v (the sample times 2^(29 - P), signed) -> v30 inside [0, Vmax]
DEV_INLINE uint32_t rsz_cubic_v30(int32_t v, uint32_t P)
{
    const int32_t top = (int32_t)(((1u << P) - 1u) << (29u - P));
    return (uint32_t)(v < 0 ? 0 : v > top ? top : v) << 1;
}

// the two passes of one tile at the pixel mapping, for source precision P and SC = 2 or 4 source channels
template <uint32_t P, uint32_t SC>
DEV_INLINE void rsz_cubic_pixel_tile(RszLds &lds, const debig_png_resize_cubic_task &t,
                                     const debig_png_resize_cubic_task *__restrict__ tg, const uint8_t *__restrict__ src,
                                     uint8_t *__restrict__ out, const RszAxes &ax, uint32_t tid)
{
    typedef typename RszHqWord<SC>::word_t word_t;
    constexpr uint32_t M = (1u << P) - 1u, HALF = M >> 1, S = 30u - P, VMAX = M << S;
    const uint32_t tw = t.tile_w;
    const word_t *hqw = reinterpret_cast<const word_t *>(lds.hq);
    if (t.mode == RSZ_ALPHA_STRAIGHT) rsz_pixel_pass1<P, SC, false, true>(lds, t, src, ax.mtx, tid);
    else rsz_pixel_pass1<P, SC, true, true>(lds, t, src, ax.mtx, tid);
    __syncthreads();
    // ---- pass 2: v_c = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c] - 2^28; the clamps; OVER adds the background's share
    const uint32_t n2 = t.tile_h * tw;
    for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
        const uint32_t yy = i / tw, x = i - yy * tw;
        const uint32_t Y = t.tile_y + yy, fy = ax.ty[2u + 2u * Y], cnt = ax.ty[3u + 2u * Y];
        const int16_t *w = ax.wyg + (uint64_t)Y * ax.mty;
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
                                      uint8_t *__restrict__ out, const RszAxes &ax, uint32_t tid)
{
    typedef typename RszSample<P>::sample_t sample_t;
    const uint32_t ch = t.channels, twc = t.tile_w * ch;
    // ---- pass 1: item (source row r, column x, channel c), c fastest: the walk of rsz_sample_pass1, signed and at a fixed P
    {
        const uint32_t n1 = t.src_rows * twc;
        StageWalk wk(tid, twc, RSZ_THREADS);
        for (uint32_t i = tid; i < n1; i += RSZ_THREADS) {
            const uint32_t x = rsz_div_ch(wk.x, ch), c = wk.x - x * ch, cnt = lds.cx[x];
            const int16_t *w = &lds.wx[x * ax.mtx];
            const sample_t *p = reinterpret_cast<const sample_t *>(src + t.src_off) + (uint64_t)(t.src_y0 + wk.r) * t.src_pitch +
                                (uint64_t)lds.fx[x] * ch + c;
            int32_t acc = 0;
            for (uint32_t k = 0; k < cnt; k++) acc += (int32_t)w[k] * (int32_t)p[(uint64_t)k * ch];
            lds.hq[i] = (uint16_t)rsz_cubic_hq(acc, P);
            wk.next();
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
        const uint32_t Y = t.tile_y + yy, fy = ax.ty[2u + 2u * Y], cnt = ax.ty[3u + 2u * Y];
        const int16_t *w = ax.wyg + (uint64_t)Y * ax.mty;
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
        // This kernel keeps the top of a tile spelled out (the text of rsz_tile_begin): with the call, before or behind its own
        // tests, the compiler lays its six tiles out differently and it ran 1 to 2 % slower (profiles/png_stage_kernels_refactor.txt)
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
        const RszAxes ax = { ty, wyg, mtx, mty };
        if (t.bits == 8u) {
            if (sc == 4u) rsz_cubic_pixel_tile<8u, 4u>(lds, t, &tasks[ti], src, out, ax, tid);
            else if (sc == 2u) rsz_cubic_pixel_tile<8u, 2u>(lds, t, &tasks[ti], src, out, ax, tid);
            else rsz_cubic_sample_tile<8u>(lds, t, &tasks[ti], src, out, ax, tid);
        } else {
            if (sc == 4u) rsz_cubic_pixel_tile<16u, 4u>(lds, t, &tasks[ti], src, out, ax, tid);
            else if (sc == 2u) rsz_cubic_pixel_tile<16u, 2u>(lds, t, &tasks[ti], src, out, ax, tid);
            else rsz_cubic_sample_tile<16u>(lds, t, &tasks[ti], src, out, ax, tid);
        }
    }
}
