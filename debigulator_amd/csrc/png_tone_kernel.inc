// png_tone_kernel.inc -- tone curves of the tensor decode: the per-channel histogram of an image's 8-bit intermediate, and the
// 256-entry table per colour channel applied to it, with the ONE conversion of the resize kernels behind it
// (include/decode_png.h: debig_png_decode_batch_tensor_tone, which has the rule; include/debig_hip.h:
// debig_hip_png_tone_hist_batch, debig_hip_png_tone_apply_batch).
//
// The first stage (a resize or warp kernel, unchanged) has written every tone file as UINT8 HWC into an arena of its own.  One
// TASK of either kernel here is a run of pix_n pixels of one such image, row major from pix0; one workgroup of 256 lanes per task.
//
// debig_png_tone_hist_kernel (AUTOCONTRAST and EQUALIZE files only):
//   - the run is a byte range that starts on a pixel, so byte k of it belongs to channel k mod channels.  The lanes read it in
//     16-byte units at 16-byte aligned addresses (uint4), the bytes in front of the first and behind the last unit one by one
//     (at most 15 each): an RGB8 run, whose pixels are 3 bytes apart, costs no byte loads beyond those;
//   - a unit's first channel is (its offset in the run) mod channels, then the channel steps with the byte; the alpha byte of
//     RGBA / GRAY_ALPHA (channel == colour_channels) is not counted;
//   - counts go to LDS with atomicAdd, one set of colour_channels x 256 counters per WAVEFRONT (4 x 3 x 256 x 4 B = 12 KB): a flat
//     image, where every lane hits one bin, contends only inside a wavefront;
//   - after a barrier the four sets are summed and the non-zero bins are added to the image's counters in global memory with
//     atomicAdd whose result is not used (at most 768 per task); the lane that flushes a counter clears it for the next task.
//   Integer adds commute: the histogram is exact whatever the order.  Nothing waits on another workgroup.
//
// debig_png_tone_apply_kernel (every tone file):
//   - the workgroup holds the image's colour_channels x 256 table in LDS.  Lane i owns entry i of every channel.  AUTOCONTRAST /
//     EQUALIZE: it reads h_c[i]; the non-empty bins of a wavefront are one ballot, the running count one inclusive scan by
//     shuffles; four ballots and four wavefront totals per channel cross through LDS, then every lane has lo, hi, the number of
//     non-empty bins, the total and its exclusive prefix, and writes its entry by the rule.  Other ops: it copies the uploaded
//     table (one table for every channel).  The table is rebuilt only when the task's (op, histogram / table offset) differs from
//     the one held, as the colour-label kernel does with its map;
//   - then one lane per pixel, lanes along x and on into the next row: it reads the pixel (one load for 1, 2 and 4 channels,
//     three bytes for RGB), maps the colour channels through LDS, passes alpha through, converts v = entry << 22 with
//     rsz_cubic_store (a[] / b[] through tg, the task in global memory) and stores with the task's strides.
// A task that breaks a bound is skipped (never indexed out of range).  No scratch, no inline assembly, plain vector stores.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_resize_kernel.inc in front of it.

#define TONE_THREADS 256u
#define TONE_AUTOCONTRAST 1u // decode_png.h: DEBIG_PNG_TONE_AUTOCONTRAST
#define TONE_EQUALIZE 2u     // decode_png.h: DEBIG_PNG_TONE_EQUALIZE
#define TONE_TABLE 5u        // decode_png.h: DEBIG_PNG_TONE_TABLE (the last op)

// the bounds both kernels share
DEV_INLINE bool tone_task_ok(const debig_png_tone_task &t)
{
    if (t.out_w == 0u || t.out_w > 16384u || t.out_h == 0u || t.out_h > 16384u || t.pix_n == 0u || t.pix_n > DEBIG_PNG_TONE_MAX_RUN)
        return false;
    const uint32_t px = t.out_w * t.out_h;
    if (t.pix0 >= px || t.pix_n > px - t.pix0) return false;
    if (t.channels == 0u || t.channels > 4u || t.colour_channels != (t.channels & 1u ? t.channels : t.channels - 1u)) return false;
    if (t.dtype > 3u || t.op == 0u || t.op > TONE_TABLE || ((t.hist_off | t.lut_off) & 15u)) return false;
    return (t.src_off & (t.channels == 3u ? 0u : t.channels - 1u)) == 0u; // (a pixel of 2 or 4 bytes is one aligned load)
}

// byte b of the run, of channel c: counted unless it is alpha
DEV_INLINE void tone_count(uint32_t *h, uint32_t b, uint32_t c, uint32_t cc)
{
    if (c < cc) atomicAdd(&h[c * 256u + b], 1u);
}

__global__ void __launch_bounds__(TONE_THREADS)
debig_png_tone_hist_kernel(const uint8_t *__restrict__ src, uint32_t *__restrict__ hist, const debig_png_tone_task *__restrict__ tasks,
                           uint32_t n_tasks)
{
    __shared__ uint32_t lds_h[4u * 768u]; /* [wavefront][channel][bin] */
    const uint32_t tid = threadIdx.x;
    uint32_t *mine = lds_h + (tid >> 6) * 768u;
    for (uint32_t k = tid; k < 4u * 768u; k += TONE_THREADS) lds_h[k] = 0u;
    __syncthreads();
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_tone_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!tone_task_ok(t) || (t.op != TONE_AUTOCONTRAST && t.op != TONE_EQUALIZE)) continue;
        const uint32_t ch = t.channels, cc = t.colour_channels;
        const uint8_t *p = src + t.src_off + (uint64_t)t.pix0 * ch;
        const uint32_t nb = t.pix_n * ch; /* <= 4 * DEBIG_PNG_TONE_MAX_RUN */
        uint32_t head = (uint32_t)(16u - ((uintptr_t)p & 15u)) & 15u;
        if (head > nb) head = nb;
        const uint32_t units = (nb - head) >> 4, tail0 = head + (units << 4);
        if (tid < head) tone_count(mine, p[tid], tid % ch, cc);
        if (tid >= 16u && tid - 16u < nb - tail0) { /* (other lanes than the head's) */
            const uint32_t k = tail0 + tid - 16u;
            tone_count(mine, p[k], k % ch, cc);
        }
        for (uint32_t u = tid; u < units; u += TONE_THREADS) {
            const uint32_t k0 = head + (u << 4);
            const uint4 q = *reinterpret_cast<const uint4 *>(p + k0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            uint32_t c = k0 % ch;
DEV_UNROLL
            for (uint32_t j = 0; j < 16u; j++) {
                tone_count(mine, (w[j >> 2] >> (8u * (j & 3u))) & 255u, c, cc);
                c = c + 1u == ch ? 0u : c + 1u;
            }
        }
        __syncthreads();
        uint32_t *g = hist + (t.hist_off >> 2);
        for (uint32_t k = tid; k < cc * 256u; k += TONE_THREADS) {
            const uint32_t s = lds_h[k] + lds_h[768u + k] + lds_h[1536u + k] + lds_h[2304u + k];
            lds_h[k] = lds_h[768u + k] = lds_h[1536u + k] = lds_h[2304u + k] = 0u;
            if (s != 0u) atomicAdd(&g[k], s);
        }
        __syncthreads();
    }
}

// entry i of one channel's table from the histogram facts every lane holds (decode_png.h has the rule): lo / hi the lowest /
// highest non-empty bin, nz their number, total the sum of all bins, h_hi the count of bin hi, ex the sum of the bins below i
DEV_INLINE uint32_t tone_entry(uint32_t op, uint32_t i, uint32_t lo, uint32_t hi, uint32_t nz, uint32_t total, uint32_t h_hi, uint32_t ex)
{
    if (op == TONE_AUTOCONTRAST) {
        if (nz == 0u || hi <= lo) return i;
        if (i < lo) return 0u;
        const uint32_t v = ((i - lo) * 255u) / (hi - lo);
        return v < 255u ? v : 255u;
    }
    const uint32_t step = (total - h_hi) / 255u;
    if (nz < 2u || step == 0u) return i;
    const uint32_t v = (step / 2u + ex) / step;
    return v < 255u ? v : 255u;
}

// the pixels of one task; CH: the channels of a pixel
template <uint32_t CH>
DEV_INLINE void tone_pixels(const uint8_t *lut, const debig_png_tone_task &t, const debig_png_tone_task *__restrict__ tg,
                            const uint8_t *__restrict__ src, uint8_t *__restrict__ out, uint32_t tid)
{
    constexpr uint32_t CC = CH & 1u ? CH : CH - 1u;
    const uint8_t *s = src + t.src_off;
    uint8_t *o = out + t.out_off;
    const uint32_t i0 = t.pix0 + tid;
    uint32_t Y = i0 / t.out_w, X = i0 - Y * t.out_w;
    const uint32_t dr = TONE_THREADS / t.out_w, dx = TONE_THREADS - dr * t.out_w;
    for (uint32_t i = tid; i < t.pix_n; i += TONE_THREADS) {
        const uint64_t at = (uint64_t)(t.pix0 + i) * CH;
        uint32_t px;
        if (CH == 4u) px = *reinterpret_cast<const uint32_t *>(s + at);
        else if (CH == 2u) px = *reinterpret_cast<const uint16_t *>(s + at);
        else if (CH == 3u) px = (uint32_t)s[at] | ((uint32_t)s[at + 1u] << 8) | ((uint32_t)s[at + 2u] << 16);
        else px = s[at];
        const uint64_t el = (uint64_t)X * t.out_sx + (uint64_t)Y * t.out_sy;
DEV_UNROLL
        for (uint32_t c = 0; c < CH; c++) {
            uint32_t v = (px >> (8u * c)) & 255u;
            if (c < CC) v = lut[c * 256u + v];
            rsz_cubic_store(t.dtype, 8u, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, v << 22);
        }
        Y += dr;
        X += dx;
        if (X >= t.out_w) { X -= t.out_w; Y++; }
    }
}

__global__ void __launch_bounds__(TONE_THREADS)
debig_png_tone_apply_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const debig_png_tone_task *__restrict__ tasks,
                            const uint32_t *__restrict__ hist, const uint8_t *__restrict__ tables, uint32_t n_tasks)
{
    __shared__ uint8_t lds_lut[768];
    __shared__ uint64_t lds_nz[12];  /* [channel][wavefront]: the ballot of its non-empty bins */
    __shared__ uint32_t lds_sum[12]; /* [channel][wavefront]: the sum of its bins */
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint64_t held_off = ~(uint64_t)0; /* the table in LDS: none yet */
    uint32_t held_op = 0u;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_tone_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!tone_task_ok(t)) continue;
        const bool from_hist = t.op == TONE_AUTOCONTRAST || t.op == TONE_EQUALIZE;
        if (from_hist && !hist) continue;
        const uint32_t cc = t.colour_channels;
        const uint64_t key = from_hist ? t.hist_off : t.lut_off;
        if (key != held_off || t.op != held_op) {
            __syncthreads(); /* nobody still reads the table that goes */
            if (from_hist) {
                uint32_t h[3], inc[3];
DEV_UNROLL
                for (uint32_t c = 0; c < 3u; c++) {
                    if (c >= cc) break; /* (uniform) */
                    h[c] = hist[(t.hist_off >> 2) + c * 256u + tid];
                    uint32_t s = h[c];
DEV_UNROLL
                    for (uint32_t d = 1u; d < 64u; d <<= 1) {
                        const uint32_t up = __shfl_up(s, d);
                        if (lane >= d) s += up;
                    }
                    inc[c] = s;
                    const uint64_t m = __ballot(h[c] != 0u);
                    if (lane == 63u) lds_sum[c * 4u + wv] = s;
                    if (lane == 0u) lds_nz[c * 4u + wv] = m;
                }
                __syncthreads();
DEV_UNROLL
                for (uint32_t c = 0; c < 3u; c++) {
                    if (c >= cc) break;
                    uint32_t lo = 0u, hi = 0u, nz = 0u, total = 0u, ex = inc[c] - h[c];
DEV_UNROLL
                    for (uint32_t w = 0; w < 4u; w++) {
                        const uint64_t m = lds_nz[c * 4u + w];
                        const uint32_t sw = lds_sum[c * 4u + w];
                        if (m != 0u) {
                            if (nz == 0u) lo = w * 64u + (uint32_t)__ffsll((unsigned long long)m) - 1u;
                            hi = w * 64u + 63u - (uint32_t)__clzll((long long)m);
                        }
                        nz += (uint32_t)__popcll(m);
                        total += sw;
                        if (w < wv) ex += sw;
                    }
                    const uint32_t h_hi = nz ? hist[(t.hist_off >> 2) + c * 256u + hi] : 0u;
                    lds_lut[c * 256u + tid] = (uint8_t)tone_entry(t.op, tid, lo, hi, nz, total, h_hi, ex);
                }
            } else {
                const uint8_t e = tables[t.lut_off + tid];
                for (uint32_t c = 0; c < cc; c++) lds_lut[c * 256u + tid] = e;
            }
            __syncthreads();
            held_off = key;
            held_op = t.op;
        }
        if (t.channels == 1u) tone_pixels<1u>(lds_lut, t, &tasks[ti], src, out, tid);
        else if (t.channels == 2u) tone_pixels<2u>(lds_lut, t, &tasks[ti], src, out, tid);
        else if (t.channels == 3u) tone_pixels<3u>(lds_lut, t, &tasks[ti], src, out, tid);
        else tone_pixels<4u>(lds_lut, t, &tasks[ti], src, out, tid);
    }
}
