// png_persp_kernel.inc -- the four warp kernels under a PROJECTIVE map (keystone, homography): crop + perspective warp of decoded
// PNG pixels into one dense tensor, with or without the colour matrix, and of raw and colour-coded labels into one dense integer
// tensor (include/decode_png.h: debig_png_decode_batch_tensor_persp, debig_png_decode_batch_labels_persp,
// debig_png_decode_batch_color_labels_persp; include/debig_hip.h: debig_hip_png_persp_batch, debig_hip_png_persp_color_batch,
// debig_hip_png_label_persp_batch, debig_hip_png_color_label_persp_batch).
//
// The arithmetic is fixed by decode_png.h: the numerators NU, NV are the affine U, V of the task's six int64 (below 2^48 in
// magnitude), the denominator D = p0 cx + p1 cy + 2 p2 is Q31 and lies in [2^21, 2^33 - 1] on the whole output, and the source
// position is U = floor(NU 2^31 / D) in Q17 (below 2^59 in magnitude), V likewise -- each by one floor division, one remainder and
// one unsigned division, all in 64 bits (persp_div).  Everything behind (U, V) is the affine warp's, word for word: the row bodies
// of png_warp_kernel.inc, png_color_kernel.inc and png_color_label_warp_kernel.inc are instantiated with the walk of this file
// (WarpPersp), so picks, taps, weights, borders, the colour mix, the LUT in LDS, the table probe and the per-wavefront
// `unmatched` add exist once.
//   - a TASK is the warp task of the kernel it mirrors, field for field, followed by int64 p[3]; tasks, workgroups and the lane
//     mapping are the warp kernels' (one lane per output pixel, lanes along X and on into the next row, 256 lanes);
//   - D is linear in X and Y, so its range over the out_w x out_h output is checked at the four corner pixels, once per task
//     and uniform over the workgroup; a task that fails it is skipped like any other bound.  Behind that check no pixel divides by
//     zero or meets a horizon, and there is no special case under CLAMP: a far-away (U, V) is an out-of-crop position like any
//     other, compared in int64 before it is narrowed;
//   - four 64-bit divisions per pixel, written with the plain operators (DESIGN.md has what they cost next to the affine twin).
// A task that breaks a bound -- those of its warp counterpart, |p_k| > 2^32, the D range -- is skipped (never indexed out of
// range).  No scratch, no inline assembly, plain vector stores only.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_warp_kernel.inc, png_color_kernel.inc and
// png_color_label_warp_kernel.inc in front of it.

#define PERSP_D_MIN ((int64_t)1 << 21)
#define PERSP_D_MAX (((int64_t)1 << 33) - 1)

// floor(N 2^31 / D) for |N| < 2^48 and D in [2^21, 2^33): q1 = floor(N / D) (|q1| <= 2^27), r1 = N - q1 D in [0, D), then
// q1 2^31 + floor(r1 2^31 / D) with r1 2^31 < 2^64
DEV_INLINE int64_t persp_div(int64_t N, int64_t D)
{
    int64_t q1 = N / D, r1 = N - q1 * D;
    if (r1 < 0) { q1--; r1 += D; } // (the operator truncates: floor for a negative N with a remainder)
    return q1 * ((int64_t)1 << 31) + (int64_t)(((uint64_t)r1 << 31) / (uint64_t)D);
}

// the limits on p[] and the range of D over the whole output, at its four corner pixels (D is linear in X and Y)
template <class Task>
DEV_INLINE bool persp_ok(const Task &t)
{
    const int64_t lim = (int64_t)1 << 32;
    if (t.p[0] < -lim || t.p[0] > lim || t.p[1] < -lim || t.p[1] > lim || t.p[2] < -lim || t.p[2] > lim) return false;
    const int64_t x1 = 2 * (int64_t)t.out_w - 1, y1 = 2 * (int64_t)t.out_h - 1; // cx, cy of the last pixel (out_w, out_h <= 16384)
    const int64_t d00 = t.p[0] + t.p[1] + 2 * t.p[2], d10 = t.p[0] * x1 + t.p[1] + 2 * t.p[2];
    const int64_t d01 = t.p[0] + t.p[1] * y1 + 2 * t.p[2], d11 = t.p[0] * x1 + t.p[1] * y1 + 2 * t.p[2];
    return d00 >= PERSP_D_MIN && d00 <= PERSP_D_MAX && d10 >= PERSP_D_MIN && d10 <= PERSP_D_MAX && d01 >= PERSP_D_MIN &&
           d01 <= PERSP_D_MAX && d11 >= PERSP_D_MIN && d11 <= PERSP_D_MAX;
}

// the output pixels of one task as warp_walk hands them out, (U, V) through the division; the caller has checked persp_ok
template <class Task, class Body>
DEV_INLINE void persp_walk(const Task &t, uint32_t tid, Body body)
{
    const uint32_t n = t.rows * t.out_w;
    StageWalk wk(tid, t.out_w, WARP_THREADS);
    for (uint32_t i = tid; i < n; i += WARP_THREADS) {
        const uint32_t X = wk.x, Y = t.row0 + wk.r;
        const int64_t cx = 2 * (int64_t)X + 1, cy = 2 * (int64_t)Y + 1;
        const int64_t D = t.p[0] * cx + t.p[1] * cy + 2 * t.p[2];
        body(X, Y, persp_div(t.m[0] * cx + t.m[1] * cy + 2 * t.m[2], D), persp_div(t.m[3] * cx + t.m[4] * cy + 2 * t.m[5], D));
        wk.next();
    }
}

struct WarpPersp {
    template <class Task, class Body>
    static DEV_MEMBER_INLINE void walk(const Task &t, uint32_t tid, Body body) { persp_walk(t, tid, body); }
};

// ---- the four kernels: each is its warp twin with the walk replaced and persp_ok among the skips -------------------------------

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_persp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const debig_png_persp_task *__restrict__ tasks,
                       uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_persp_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || t.channels == 0u || t.channels > 4u ||
            (t.bits != 8u && t.bits != 16u) || t.dtype > 3u || (t.filter != WARP_FILTER_BILINEAR && t.filter != WARP_FILTER_NEAREST) ||
            t.border_mode > WARP_BORDER_CLAMP || !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) ||
            (t.src_off & ((uint32_t)t.bits / 8u - 1u)) || !persp_ok(t))
            continue;
        if (t.bits == 8u) warp_rows<8u, WarpPersp>(t, &tasks[ti], src, out, tid);
        else warp_rows<16u, WarpPersp>(t, &tasks[ti], src, out, tid);
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_persp_color_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                             const debig_png_persp_color_task *__restrict__ tasks, const uint8_t *__restrict__ weights, uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_persp_color_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || (t.channels != 3u && t.channels != 4u) ||
            (t.bits != 8u && t.bits != 16u) || t.dtype > 3u || (t.filter != WARP_FILTER_BILINEAR && t.filter != WARP_FILTER_NEAREST) ||
            t.border_mode > WARP_BORDER_CLAMP || !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) ||
            (t.src_off & ((uint32_t)t.bits / 8u - 1u)) || (t.color_off & 7u) || !persp_ok(t))
            continue;
        const debig_png_color_rec cr = *reinterpret_cast<const debig_png_color_rec *>(weights + t.color_off);
        if (!color_rec_ok(cr, t.bits)) continue;
        if (t.bits == 8u) warp_color_rows<8u, WarpPersp>(t, &tasks[ti], cr, src, out, tid);
        else warp_color_rows<16u, WarpPersp>(t, &tasks[ti], cr, src, out, tid);
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_label_persp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                             const debig_png_label_persp_task *__restrict__ tasks, const int32_t *__restrict__ lut, uint32_t n_tasks)
{
    __shared__ int32_t lds_lut[256];
    const uint32_t tid = threadIdx.x;
    if (lut) lds_lut[tid & 255u] = lut[tid & 255u];
    __syncthreads();
    const int32_t *L = lut ? lds_lut : nullptr;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_persp_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || (t.src_bytes != 1u && t.src_bytes != 2u) ||
            t.dtype > 3u || (t.dtype == 0u && t.src_bytes == 2u) || (lut && t.src_bytes == 2u) || t.border_mode > WARP_BORDER_CLAMP ||
            !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) || (t.src_off & (t.src_bytes - 1u)) || !persp_ok(t))
            continue;
        if (t.src_bytes == 1u) {
            if (t.dtype == 0u) warp_label_rows<1u, 1u, WarpPersp>(L, t, src, out, tid);
            else if (t.dtype == 1u) warp_label_rows<2u, 1u, WarpPersp>(L, t, src, out, tid);
            else if (t.dtype == 2u) warp_label_rows<4u, 1u, WarpPersp>(L, t, src, out, tid);
            else warp_label_rows<8u, 1u, WarpPersp>(L, t, src, out, tid);
        } else {
            if (t.dtype == 1u) warp_label_rows<2u, 2u, WarpPersp>(L, t, src, out, tid);
            else if (t.dtype == 2u) warp_label_rows<4u, 2u, WarpPersp>(L, t, src, out, tid);
            else warp_label_rows<8u, 2u, WarpPersp>(L, t, src, out, tid);
        }
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_color_label_persp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                                   const debig_png_color_label_persp_task *__restrict__ tasks, const uint8_t *__restrict__ tables,
                                   uint32_t *__restrict__ unmatched, uint32_t n_tasks)
{
    __shared__ uint2 lds_map[DEBIG_PNG_CMAP_MAX_SLOTS]; /* (key, value) per slot */
    const uint2 *tab = lds_map;
    const uint32_t tid = threadIdx.x;
    ClblHeld held = { ~(uint64_t)0, 0u };
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_color_label_persp_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || t.dtype > 3u || t.mode > 1u ||
            t.border_mode > WARP_BORDER_CLAMP || !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) || !persp_ok(t))
            continue;
        if (t.mode == 0u ? t.dtype < 2u
                         : (t.map_slots < 2u || t.map_slots > DEBIG_PNG_CMAP_MAX_SLOTS || (t.map_slots & (t.map_slots - 1u)) ||
                            (t.map_off & 15u) || !unmatched))
            continue;
        if (t.mode == 0u) {
            if (t.dtype == 2u) clbl_warp_rows<4u, false, WarpPersp>(tab, t, src, out, tid);
            else clbl_warp_rows<8u, false, WarpPersp>(tab, t, src, out, tid);
            continue;
        }
        clbl_hold_map(lds_map, held, t, tables, tid);
        uint32_t m;
        if (t.dtype == 0u) m = clbl_warp_rows<1u, true, WarpPersp>(tab, t, src, out, tid);
        else if (t.dtype == 1u) m = clbl_warp_rows<2u, true, WarpPersp>(tab, t, src, out, tid);
        else if (t.dtype == 2u) m = clbl_warp_rows<4u, true, WarpPersp>(tab, t, src, out, tid);
        else m = clbl_warp_rows<8u, true, WarpPersp>(tab, t, src, out, tid);
        clbl_add_misses(&unmatched[t.image], m, tid);
    }
}
