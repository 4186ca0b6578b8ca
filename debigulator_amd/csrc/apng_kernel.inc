// apng_kernel.inc -- APNG compositing (include/decode_png.h: debig_apng_decode_batch; include/debig_hip.h:
// debig_hip_apng_composite_batch).
//
// Per canvas pixel the APNG rules are a scan over the file's frames with O(1) state: the current pixel and the one saved
// for dispose_op PREVIOUS.  One TASK is a slice of at most DEBIG_APNG_TASK_PX pixels of one canvas; one workgroup of 256
// lanes per task, lane l owns the 4 consecutive canvas pixels px0 + 4l .. px0 + 4l + 3, keeps both values in registers
// and loops over the frames:
//   - the frame table (uniform per workgroup) is read once per frame;
//   - a pixel inside the frame's region reads its source pixel as a dword (x_off makes a run unaligned to 16 bytes; when
//     the lane's 4 pixels lie in one row of the region the 4 dwords are adjacent);
//   - every pixel is stored into canvas k, in the widest stores the slot's alignment allows (spec_store_run of
//     png_spec_kernel.inc): each frame's pixels are read once and each output byte is written once, no LDS.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_spec_kernel.inc in front of it.

#define APNG_THREADS 256u
#define APNG_RUN 4u /* pixels per lane: APNG_THREADS * APNG_RUN == DEBIG_APNG_TASK_PX */

// num / al for num <= 255 * al < 2^24 (exact in fp32): a reciprocal estimate, corrected to the truncated quotient
DEV_INLINE uint32_t apng_div(uint32_t num, uint32_t al, float rcp)
{
    uint32_t q = (uint32_t)((float)num * rcp);
    if (q * al > num) q--;
    else if ((q + 1u) * al <= num) q++;
    return q;
}

// s OVER d (decode_png.h: integer form of the APNG specification's rule)
DEV_INLINE uint32_t apng_over(uint32_t s, uint32_t d)
{
    const uint32_t sa = s >> 24;
    if (sa == 255u) return s;
    if (sa == 0u) return d;
    const uint32_t u = sa * 255u, v = (255u - sa) * (d >> 24), al = u + v;
    const float rcp = 1.0f / (float)al;
    uint32_t r = 0u;
DEV_UNROLL
    for (uint32_t c = 0; c < 24u; c += 8u)
        r |= apng_div(((s >> c) & 255u) * u + ((d >> c) & 255u) * v, al, rcp) << c;
    return r | (apng_div(al, 255u, 1.0f / 255.0f) << 24);
}

__global__ void __launch_bounds__(APNG_THREADS)
debig_apng_composite_kernel(const uint8_t *__restrict__ frames, uint8_t *__restrict__ out,
                            const debig_apng_task *__restrict__ tasks, uint32_t n_tasks)
{
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_apng_task t = tasks[ti];
        const uint32_t j0 = (uint32_t)threadIdx.x * APNG_RUN;
        if (j0 >= t.n_px) continue;
        const uint32_t np = t.n_px - j0 < APNG_RUN ? t.n_px - j0 : APNG_RUN;
        const uint64_t p0 = t.px0 + j0;
        uint32_t xs[APNG_RUN], ys[APNG_RUN];
        {
            uint32_t y = (uint32_t)(p0 / t.width), x = (uint32_t)(p0 - (uint64_t)y * t.width);
DEV_UNROLL
            for (uint32_t j = 0; j < APNG_RUN; j++) {
                xs[j] = x;
                ys[j] = y;
                if (++x == t.width) { x = 0u; y++; }
            }
        }
        const uint64_t plane = (uint64_t)t.width * t.height * 4u;
        uint8_t *o = out + t.out_off + p0 * 4u;
        const debig_apng_frame_desc *ft = reinterpret_cast<const debig_apng_frame_desc *>(frames + t.ftab_off);
        uint32_t cur[APNG_RUN], sav[APNG_RUN];
DEV_UNROLL
        for (uint32_t j = 0; j < APNG_RUN; j++) cur[j] = sav[j] = 0u;
        for (uint32_t k = 0; k < t.n_frames; k++, o += plane) {
            const debig_apng_frame_desc f = ft[k];
            const uint32_t dop = k == 0u && f.dispose_op == 2u ? 1u : f.dispose_op;
            const uint32_t *src = reinterpret_cast<const uint32_t *>(frames + f.rgba_off);
            uint32_t in = 0u; // pixels of the run inside the region
            uint32_t s[APNG_RUN];
            const uint32_t cx0 = xs[0] - f.x_off, cy0 = ys[0] - f.y_off; // (unsigned: left of / above the region wraps)
            if (np == APNG_RUN && ys[APNG_RUN - 1u] == ys[0] && cy0 < f.height && cx0 < f.width && cx0 + APNG_RUN <= f.width) {
                // the whole run in one row of the region: 4 adjacent dwords
                const uint32_t *q = src + (uint64_t)cy0 * f.width + cx0;
DEV_UNROLL
                for (uint32_t j = 0; j < APNG_RUN; j++) s[j] = q[j];
                in = (1u << APNG_RUN) - 1u;
            } else {
DEV_UNROLL
                for (uint32_t j = 0; j < APNG_RUN; j++) {
                    const uint32_t cx = xs[j] - f.x_off, cy = ys[j] - f.y_off;
                    s[j] = 0u;
                    if (j < np && cx < f.width && cy < f.height) {
                        s[j] = src[(uint64_t)cy * f.width + cx];
                        in |= 1u << j;
                    }
                }
            }
DEV_UNROLL
            for (uint32_t j = 0; j < APNG_RUN; j++) {
                if (!((in >> j) & 1u)) continue;
                if (dop == 2u) sav[j] = cur[j];
                cur[j] = f.blend_op ? apng_over(s[j], cur[j]) : s[j];
            }
            if (np == APNG_RUN) {
                spec_store_run<4u * APNG_RUN>(o, cur);
            } else {
DEV_UNROLL
                for (uint32_t j = 0; j < APNG_RUN; j++)
                    if (j < np) spec_store_run<4u>(o + 4u * j, &cur[j]);
            }
DEV_UNROLL
            for (uint32_t j = 0; j < APNG_RUN; j++) {
                if (!((in >> j) & 1u)) continue;
                if (dop == 1u) cur[j] = 0u;
                else if (dop == 2u) cur[j] = sav[j];
            }
        }
    }
}
