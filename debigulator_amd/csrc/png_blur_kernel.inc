// png_blur_kernel.inc -- Gaussian blur and sharpness of the tensor decode: a separable convolution (or the 3 x 3 SMOOTH and a
// blend) on an image's 8-bit intermediate, with the ONE conversion of the resize kernels behind it
// (include/decode_png.h: debig_png_decode_batch_tensor_blur, which has the rule; include/debig_hip.h: debig_hip_png_blur_batch).
//
// The stages in front (a resize or warp kernel and, for a file that has a tone operation too, the tone apply kernel; all
// unchanged) have written every blur file as UINT8 HWC into an arena.  One TASK is a tile of tile_w x tile_h output pixels of one
// such image; one workgroup of 256 lanes per task:
//   - lanes below tile_w + 2 radius fold the tile's source columns x0 - radius .. by the mirror rule (period 2 (n - 1), n == 1:
//     always 0), lanes from 128 on its rows, into two small LDS tables: the only place where an index is folded;
//   - GAUSSIAN: the file's weights go to LDS, only when the task's table offset differs from the one held (as the tone and
//     colour-label kernels do with their tables);
//   - the tile with its halo goes to LDS as bytes, one pixel per lane and step (one load for 1, 2 and 4 channels, three bytes for
//     RGB), lanes along the row and on into the next;
//   - GAUSSIAN, horizontal: item e = (row of the haloed tile, x, c), c fastest, lanes along e: a lane reads bytes `channels`
//     apart, neighbouring lanes read neighbouring bytes; h16 = (sum + 32) >> 6 goes to the 16-bit plane at e.  Vertical: one item
//     per output element, walking DOWN the plane; v is the sample in Q22 and goes to rsz_cubic_store.  The weights are read two
//     to a 32-bit LDS word, the odd last one alone;
//   - SHARPNESS: one item per output element; the nine bytes come from the byte tile (halo 1); elements on the image's one-pixel
//     border ring and alpha keep their sample; the blend is in 64-bit integers;
//   - items of the last pass are (y, x, c) with c fastest when the output's channel stride is 1 (HWC: adjacent lanes store adjacent
//     elements), else (c, y, x) with x fastest (CHW: runs of tile_w adjacent elements per plane row).
// Every sum is an integer sum, so no result depends on its order.  LDS: 24 KB of h16 + 35 KB of bytes + 128 B of weights + 512 B
// of folded indices = 61,056 B, static.  A task that breaks a bound is skipped whole (never indexed out of range).  No scratch,
// no inline assembly, plain vector stores, nothing shared between workgroups.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_resize_kernel.inc in front of it.

#define BLUR_THREADS 256u
#define BLUR_GAUSSIAN 1u  // decode_png.h: DEBIG_PNG_BLUR_GAUSSIAN
#define BLUR_SHARPNESS 2u // decode_png.h: DEBIG_PNG_BLUR_SHARPNESS (the last op)

struct alignas(16) BlurLds {
    uint16_t h16[DEBIG_PNG_BLUR_H16_CAP];
    uint8_t px[DEBIG_PNG_BLUR_PX_CAP];
    uint32_t q2[32]; /* the 63 weights and a zero, two to a word */
    uint16_t fx[128], fy[128];
};

// the bounds of a task
DEV_INLINE bool blur_task_ok(const debig_png_blur_task &t)
{
    if (t.w == 0u || t.w > 16384u || t.h == 0u || t.h > 16384u) return false;
    if (t.tile_w == 0u || t.tile_w > DEBIG_PNG_BLUR_MAX_TILE || t.tile_h == 0u || t.tile_h > DEBIG_PNG_BLUR_MAX_TILE) return false;
    if (t.x0 >= t.w || t.tile_w > t.w - t.x0 || t.y0 >= t.h || t.tile_h > t.h - t.y0) return false;
    if (t.channels == 0u || t.channels > 4u || t.colour_channels != (t.channels & 1u ? t.channels : t.channels - 1u)) return false;
    if (t.dtype > 3u || t.op == 0u || t.op > BLUR_SHARPNESS || (t.table_off & 15u)) return false;
    if (t.op == BLUR_GAUSSIAN ? t.radius == 0u || t.radius > 31u : t.radius != 1u) return false;
    if (t.k > (16 << 16) || t.k < -(16 << 16)) return false;
    const uint32_t rows = t.tile_h + 2u * t.radius, cols = t.tile_w + 2u * t.radius; /* <= 126 */
    if (rows * cols * t.channels > DEBIG_PNG_BLUR_PX_CAP) return false;
    if (t.op == BLUR_GAUSSIAN && rows * t.tile_w * t.channels > DEBIG_PNG_BLUR_H16_CAP) return false;
    return (t.src_off & (t.channels == 3u ? 0u : t.channels - 1u)) == 0u; // (a pixel of 2 or 4 bytes is one aligned load)
}

// index i of an axis of n samples, mirrored without repeating the edge
DEV_INLINE uint32_t blur_fold(int32_t i, uint32_t n)
{
    if (n == 1u) return 0u;
    const int32_t last = (int32_t)n - 1;
    while (i < 0 || i > last) i = i < 0 ? -i : 2 * last - i;
    return (uint32_t)i;
}

// the tile with its halo -> lds.px, HWC; CH: the channels of a pixel
template <uint32_t CH>
DEV_INLINE void blur_load(BlurLds &lds, const debig_png_blur_task &t, const uint8_t *__restrict__ src, uint32_t tid)
{
    const uint32_t cols = t.tile_w + 2u * t.radius, n = (t.tile_h + 2u * t.radius) * cols;
    const uint8_t *s = src + t.src_off;
    uint32_t ry = tid / cols, rx = tid - ry * cols;
    const uint32_t dr = BLUR_THREADS / cols, dx = BLUR_THREADS - dr * cols;
    for (uint32_t i = tid; i < n; i += BLUR_THREADS) {
        const uint64_t at = ((uint64_t)lds.fy[ry] * t.w + lds.fx[rx]) * CH;
        if (CH == 4u) reinterpret_cast<uint32_t *>(lds.px)[i] = *reinterpret_cast<const uint32_t *>(s + at);
        else if (CH == 2u) reinterpret_cast<uint16_t *>(lds.px)[i] = *reinterpret_cast<const uint16_t *>(s + at);
        else if (CH == 3u) {
            lds.px[3u * i] = s[at];
            lds.px[3u * i + 1u] = s[at + 1u];
            lds.px[3u * i + 2u] = s[at + 2u];
        } else lds.px[i] = s[at];
        ry += dr;
        rx += dx;
        if (rx >= cols) { rx -= cols; ry++; }
    }
}

// item e of the last pass -> (x, y, c) inside the tile
template <uint32_t CH>
DEV_INLINE void blur_item(const debig_png_blur_task &t, uint32_t e, uint32_t &x, uint32_t &y, uint32_t &c)
{
    if (t.out_sc == 1u) {
        const uint32_t p = e / CH;
        c = e - p * CH;
        y = p / t.tile_w;
        x = p - y * t.tile_w;
    } else {
        const uint32_t p = e / t.tile_w;
        x = e - p * t.tile_w;
        c = p / t.tile_h;
        y = p - c * t.tile_h;
    }
}

// sum of w[j] * p[j * STEP] over the 2 r + 1 taps; p: bytes or halfwords
template <typename S>
DEV_INLINE uint32_t blur_taps(const uint32_t *q2, const S *p, uint32_t step, uint32_t r)
{
    uint32_t acc = 0u;
    for (uint32_t j = 0; j < r; j++) {
        const uint32_t w = q2[j];
        acc += (w & 0xffffu) * p[0] + (w >> 16) * p[step];
        p += 2u * step;
    }
    return acc + (q2[r] & 0xffffu) * p[0];
}

template <uint32_t CH>
DEV_INLINE void blur_gaussian(BlurLds &lds, const debig_png_blur_task &t, const debig_png_blur_task *__restrict__ tg,
                              uint8_t *__restrict__ out, uint32_t tid)
{
    const uint32_t r = t.radius, cols = t.tile_w + 2u * r, rows = t.tile_h + 2u * r, twc = t.tile_w * CH;
    for (uint32_t e = tid; e < rows * twc; e += BLUR_THREADS) {
        const uint32_t ry = e / twc;
        const uint32_t h = blur_taps(lds.q2, lds.px + ry * cols * CH + (e - ry * twc), CH, r); /* <= 255 << 14 */
        lds.h16[e] = (uint16_t)((h + 32u) >> 6);
    }
    __syncthreads();
    uint8_t *o = out + t.out_off;
    for (uint32_t e = tid; e < t.tile_h * twc; e += BLUR_THREADS) {
        uint32_t x, y, c;
        blur_item<CH>(t, e, x, y, c);
        const uint32_t v = blur_taps(lds.q2, lds.h16 + y * twc + x * CH + c, twc, r); /* <= 65280 << 14 = 255 << 22 */
        const uint64_t el = (uint64_t)(t.x0 + x) * t.out_sx + (uint64_t)(t.y0 + y) * t.out_sy + (uint64_t)c * t.out_sc;
        rsz_cubic_store(t.dtype, 8u, tg->a[c], tg->b[c], o, el, v);
    }
}

template <uint32_t CH>
DEV_INLINE void blur_sharpness(BlurLds &lds, const debig_png_blur_task &t, const debig_png_blur_task *__restrict__ tg,
                               uint8_t *__restrict__ out, uint32_t tid)
{
    constexpr uint32_t CC = CH & 1u ? CH : CH - 1u;
    const uint32_t cols = t.tile_w + 2u, twc = t.tile_w * CH;
    uint8_t *o = out + t.out_off;
    for (uint32_t e = tid; e < t.tile_h * twc; e += BLUR_THREADS) {
        uint32_t x, y, c;
        blur_item<CH>(t, e, x, y, c);
        const uint8_t *m = lds.px + ((y + 1u) * cols + x + 1u) * CH + c, *u = m - cols * CH, *d = m + cols * CH;
        const uint32_t p = m[0], X = t.x0 + x, Y = t.y0 + y;
        uint32_t v = p << 22;
        if (c < CC && X >= 1u && X + 2u <= t.w && Y >= 1u && Y + 2u <= t.h) {
            constexpr int32_t L = -(int32_t)CH, R = (int32_t)CH;
            const uint32_t sum = u[L] + u[0] + u[R] + m[L] + 5u * p + m[R] + d[L] + d[0] + d[R];
            const uint32_t s = (2u * sum + 13u) / 26u;
            const int64_t b = ((int64_t)s << 22) + (int64_t)t.k * ((int32_t)p - (int32_t)s) * 64;
            v = (uint32_t)(b < 0 ? 0 : b > ((int64_t)255 << 22) ? (int64_t)255 << 22 : b);
        }
        const uint64_t el = (uint64_t)X * t.out_sx + (uint64_t)Y * t.out_sy + (uint64_t)c * t.out_sc;
        rsz_cubic_store(t.dtype, 8u, tg->a[c], tg->b[c], o, el, v);
    }
}

template <uint32_t CH>
DEV_INLINE void blur_tile(BlurLds &lds, const debig_png_blur_task &t, const debig_png_blur_task *__restrict__ tg,
                          const uint8_t *__restrict__ src, uint8_t *__restrict__ out, uint32_t tid)
{
    blur_load<CH>(lds, t, src, tid);
    __syncthreads();
    if (t.op == BLUR_GAUSSIAN) blur_gaussian<CH>(lds, t, tg, out, tid); /* (uniform over the workgroup) */
    else blur_sharpness<CH>(lds, t, tg, out, tid);
}

__global__ void __launch_bounds__(BLUR_THREADS)
debig_png_blur_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const debig_png_blur_task *__restrict__ tasks,
                      const uint8_t *__restrict__ tables, uint32_t n_tasks)
{
    __shared__ BlurLds lds;
    const uint32_t tid = threadIdx.x;
    uint64_t held_off = ~(uint64_t)0; /* the weights in LDS: none yet */
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_blur_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!blur_task_ok(t)) continue;
        __syncthreads(); /* nobody still reads what the task before left in LDS */
        const uint32_t r = t.radius;
        if (tid < t.tile_w + 2u * r) lds.fx[tid] = (uint16_t)blur_fold((int32_t)(t.x0 + tid) - (int32_t)r, t.w);
        if (tid >= 128u && tid - 128u < t.tile_h + 2u * r) lds.fy[tid - 128u] = (uint16_t)blur_fold((int32_t)(t.y0 + tid - 128u) - (int32_t)r, t.h);
        if (t.op == BLUR_GAUSSIAN && t.table_off != held_off) {
            if (tid < 32u) {
                const uint16_t *q = reinterpret_cast<const uint16_t *>(tables + t.table_off);
                lds.q2[tid] = (uint32_t)q[2u * tid] | (tid < 31u ? (uint32_t)q[2u * tid + 1u] << 16 : 0u);
            }
            held_off = t.table_off;
        }
        __syncthreads();
        if (t.channels == 1u) blur_tile<1u>(lds, t, &tasks[ti], src, out, tid);
        else if (t.channels == 2u) blur_tile<2u>(lds, t, &tasks[ti], src, out, tid);
        else if (t.channels == 3u) blur_tile<3u>(lds, t, &tasks[ti], src, out, tid);
        else blur_tile<4u>(lds, t, &tasks[ti], src, out, tid);
    }
}
