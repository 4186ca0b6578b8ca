// png_persp_kernel.inc -- the four warp kernels under a PROJECTIVE map (keystone, homography): crop + perspective warp of decoded
// PNG pixels into one dense tensor, with or without the colour matrix, and of raw and colour-coded labels into one dense integer
// tensor (include/decode_png.h: debig_png_decode_batch_tensor_persp, debig_png_decode_batch_labels_persp,
// debig_png_decode_batch_color_labels_persp; include/debig_hip.h: debig_hip_png_persp_batch, debig_hip_png_persp_color_batch,
// debig_hip_png_label_persp_batch, debig_hip_png_color_label_persp_batch).
//
// The arithmetic is fixed by decode_png.h: the numerators NU, NV are the affine U, V of the task's six int64 (below 2^48 in
// magnitude), the denominator D = p0 cx + p1 cy + 2 p2 is Q31 and lies in [2^21, 2^33 - 1] on the whole output, and the source
// position is U = floor(NU 2^31 / D) in Q17 (below 2^59 in magnitude), V likewise -- each by one floor division, one remainder and
// one unsigned division, all in 64 bits (persp_div).  Everything around (U, V) is the affine warp's, word for word: the kernel bodies
// of png_warp_kernel.inc, png_color_kernel.inc and png_color_label_warp_kernel.inc (warp_image_tasks, warp_color_tasks,
// warp_label_tasks, clbl_warp_tasks) are instantiated with the map policy of this file (WarpPersp), so the task loop, the skips,
// the ladders, the pixel walk, picks, taps, weights, borders, the colour mix, the LUT in LDS, the table probe and the
// per-wavefront `unmatched` add exist once.
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

// the projective map as the policy the kernel bodies take (png_warp_kernel.inc has the scheme): persp_ok among the skips, nothing
// to hold, (U, V) through the division -- behind persp_ok, which the bodies have tested by then
struct WarpPersp {
    template <class Task>
    static DEV_MEMBER_INLINE bool task_ok(const Task &t) { return persp_ok(t); }
    template <class Task>
    static DEV_MEMBER_INLINE bool hold(const Task &, uint32_t) { return true; }
    template <class Task>
    static DEV_MEMBER_INLINE void uv(const Task &t, uint32_t, uint32_t, int64_t cx, int64_t cy, int64_t &U, int64_t &V)
    {
        const int64_t D = t.p[0] * cx + t.p[1] * cy + 2 * t.p[2];
        U = persp_div(warp_nu(t, cx, cy), D);
        V = persp_div(warp_nv(t, cx, cy), D);
    }
};

// ---- the four kernels: the body of each kind under the projective map -----------------------------------------------------------

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_persp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const debig_png_persp_task *__restrict__ tasks,
                       uint32_t n_tasks)
{
    warp_image_tasks(WarpPersp(), src, out, tasks, n_tasks);
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_persp_color_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                             const debig_png_persp_color_task *__restrict__ tasks, const uint8_t *__restrict__ weights, uint32_t n_tasks)
{
    warp_color_tasks(WarpPersp(), src, out, tasks, weights, n_tasks);
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_label_persp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                             const debig_png_label_persp_task *__restrict__ tasks, const int32_t *__restrict__ lut, uint32_t n_tasks)
{
    __shared__ int32_t lds_lut[256];
    warp_label_tasks(WarpPersp(), lds_lut, src, out, tasks, lut, n_tasks);
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_color_label_persp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                                   const debig_png_color_label_persp_task *__restrict__ tasks, const uint8_t *__restrict__ tables,
                                   uint32_t *__restrict__ unmatched, uint32_t n_tasks)
{
    __shared__ uint2 lds_map[DEBIG_PNG_CMAP_MAX_SLOTS]; /* (key, value) per slot */
    clbl_warp_tasks(WarpPersp(), lds_map, src, out, tasks, tables, unmatched, n_tasks);
}
