// png_warp_kernel.inc -- crop + affine warp (flips, quarter turns, rotation, scale, shear) + normalise of decoded PNG pixels into
// one dense tensor, and the same warp of raw labels into one dense integer tensor
// (include/decode_png.h: debig_png_decode_batch_tensor_warp, debig_png_decode_batch_labels_warp; include/debig_hip.h:
// debig_hip_png_warp_batch, debig_hip_png_label_warp_batch).
//
// The arithmetic is fixed by decode_png.h: the inverse map as six int64 in Q16, the source position of an output pixel's
// centre in Q17 (U, V: int64, below 2^48 in magnitude), floor shifts for the pick, Q14 weights from the low 17 bits, the
// horizontal pass rounded to 16 bits, the vertical pass into 30 bits, then the ONE conversion of the resize kernels
// (rsz_cubic_store).  An affine map is not separable, so nothing of the two-pass LDS scheme of png_resize_kernel.inc carries
// over: this is a gather.
//
// One TASK is a run of output rows of one image; one workgroup of 256 lanes per task:
//   - an ITEM is one output pixel; the lanes run along X, then on into the next row of the run, so narrow tensors keep every
//     lane busy and a wavefront's stores are adjacent pixels of a row (CHW: adjacent elements of each plane row; HWC: elements
//     `channels` apart, the channel loop fills the gaps within the same cache lines);
//   - a lane computes U and V of its pixel from the task's six int64, then per channel loads its 1 (nearest) or 4 (bilinear)
//     taps straight from the arena.  The source footprint of a row run is a thin parallelogram of the crop; neighbouring lanes
//     read neighbouring or identical samples, and the second tap row of one output row is the first of a later one: the
//     re-reads are L1 / L2 hits.  (An LDS-staged footprint was not built: profiles/png_warp.txt has the measurement of this
//     version against the two-pass torch route.)
//   - every tap index is clamped into the crop BEFORE it addresses memory, whatever the border mode; under CONSTANT the
//     loaded value is then replaced by the border sample by a select.  No lane reads outside the crop, and no branch diverges
//     on the position;
//   - a[] / b[] / border[] are read through tg, the task in global memory, where a run-time channel index costs nothing
//     (into the by-value struct it would go through scratch).
// The label kernel has the same tasks and the same U, V; its 256-entry LUT is staged in LDS once per workgroup, as in
// png_label_kernel.inc.  A border pick stores border_label as it is (it does not pass through the LUT).
// A task that breaks a bound is skipped (never indexed out of range).  No atomics, no scratch, nothing shared between
// workgroups; plain vector stores only.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_stage_common.inc in front of it.

#define WARP_THREADS 256u
#define WARP_FILTER_BILINEAR 0u // decode_png.h: DEBIG_PNG_FILTER_BILINEAR
#define WARP_FILTER_NEAREST 2u  // decode_png.h: DEBIG_PNG_FILTER_NEAREST
#define WARP_BORDER_CLAMP 1u    // decode_png.h: DEBIG_PNG_BORDER_CLAMP (0: _CONSTANT)

// the matrix limits of decode_png.h on the quantised entries: they keep |U|, |V| below 2^48
DEV_INLINE bool warp_matrix_ok(int64_t m00, int64_t m01, int64_t m02, int64_t m10, int64_t m11, int64_t m12)
{
    const int64_t lin = (int64_t)1 << 31, tr = (int64_t)1 << 40;
    return m00 >= -lin && m00 <= lin && m01 >= -lin && m01 <= lin && m10 >= -lin && m10 <= lin && m11 >= -lin && m11 <= lin &&
           m02 >= -tr && m02 <= tr && m12 >= -tr && m12 <= tr;
}

// the sizes every warp task shares.  (The two gather kernels spell the first four tests out themselves: with one predicate
// for all, the compiler lays the kernels' skips out differently; profiles/png_stage_kernels_refactor.txt has what that cost.)
DEV_INLINE bool warp_sizes_ok(uint32_t out_w, uint32_t out_h, uint32_t row0, uint32_t rows, uint32_t crop_w, uint32_t crop_h)
{
    return out_w != 0u && out_w <= 16384u && out_h <= 16384u && rows != 0u && row0 < out_h && rows <= out_h - row0 &&
           crop_w != 0u && crop_w <= 0x7fffffffu && crop_h != 0u && crop_h <= 0x7fffffffu;
}

// an index clamped into [0, cl - 1]; *inside: whether it lay there (int64 comparisons, before anything is narrowed)
DEV_INLINE uint32_t warp_clamp(int64_t j, uint32_t cl, bool *inside)
{
    *inside = j >= 0 && j < (int64_t)cl;
    return (uint32_t)(j < 0 ? 0 : j >= (int64_t)cl ? (int64_t)cl - 1 : j);
}

// ---- what the twelve warp kernels share (this file, png_color_kernel.inc, png_color_label_warp_kernel.inc, png_persp_kernel.inc,
// png_elastic_kernel.inc).  They are KIND x MAP: four kinds -- image (warp_image_tasks, here), image + colour matrix
// (warp_color_tasks, png_color_kernel.inc), label (warp_label_tasks, here), colour label (clbl_warp_tasks,
// png_color_label_warp_kernel.inc) -- which differ in what they do with a picked sample, under three maps, which differ in how
// (U, V) comes about.  A kind's body is written once, as a template over the task type and the map; a __global__ kernel declares
// its LDS and calls the body with its map, which the body takes BY VALUE (by reference the colour-label elastic kernel spilled
// three more scalar registers; profiles/png_warp_maps_refactor.txt).
//
// A MAP POLICY provides three things and nothing else:
//   task_ok(t)                     what the map adds to the bounds of a task (uniform over the workgroup); the bodies test it
//                                  last in their first predicate
//   hold(t, tid)                   the step in front of a task's walk, reached by every lane of the workgroup -> false: the task
//                                  is skipped
//   uv(t, X, Y, cx, cy, U, V)      the source position (U, V), Q17, of output pixel (X, Y) with centre (cx, cy) = (2X + 1, 2Y + 1)
// WarpAffine (below) and WarpPersp (png_persp_kernel.inc) are empty types: their hold is `true`, so their kernels have no barrier,
// no LDS and no branch of it.  WarpElastic (png_elastic_kernel.inc) carries the pointers to its grid in LDS and what it holds.
// A new map is a fourth policy and four __global__ kernels of one call each; a new kind is one body and a kernel per map.

// the affine numerators of one output pixel from the task's six int64: every map starts from them
template <class Task>
DEV_INLINE int64_t warp_nu(const Task &t, int64_t cx, int64_t cy) { return t.m[0] * cx + t.m[1] * cy + 2 * t.m[2]; }
template <class Task>
DEV_INLINE int64_t warp_nv(const Task &t, int64_t cx, int64_t cy) { return t.m[3] * cx + t.m[4] * cy + 2 * t.m[5]; }

struct WarpAffine {
    template <class Task>
    static DEV_MEMBER_INLINE bool task_ok(const Task &) { return true; }
    template <class Task>
    static DEV_MEMBER_INLINE bool hold(const Task &, uint32_t) { return true; }
    template <class Task>
    static DEV_MEMBER_INLINE void uv(const Task &t, uint32_t, uint32_t, int64_t cx, int64_t cy, int64_t &U, int64_t &V)
    {
        U = warp_nu(t, cx, cy);
        V = warp_nv(t, cx, cy);
    }
};

// the output pixels of one task, lanes along X and on into the next row of the run: body(X, Y, U, V) per pixel, (U, V) the
// source position of its centre in Q17 under the map.  The ONE pixel loop of the family
template <class Map, class Task, class Body>
DEV_INLINE void warp_walk(const Map &map, const Task &t, uint32_t tid, Body body)
{
    const uint32_t n = t.rows * t.out_w;
    StageWalk wk(tid, t.out_w, WARP_THREADS);
    for (uint32_t i = tid; i < n; i += WARP_THREADS) {
        const uint32_t X = wk.x, Y = t.row0 + wk.r;
        const int64_t cx = 2 * (int64_t)X + 1, cy = 2 * (int64_t)Y + 1;
        int64_t U, V;
        map.uv(t, X, Y, cx, cy, U, V);
        body(X, Y, U, V);
        wk.next();
    }
}

// the NEAREST pick of (U, V): the pixel (jx, jy), clamped into the crop, and whether its sample counts -- under CLAMP always,
// under CONSTANT when the pick lay inside (else the border value takes its place, by a select).  clamp: the task's border mode
// is CLAMP, found once per task by the caller, in front of its walk
struct WarpPick {
    uint32_t jx, jy;
    bool keep;
};
template <class Task>
DEV_INLINE WarpPick warp_pick(const Task &t, bool clamp, int64_t U, int64_t V)
{
    bool inx, iny;
    WarpPick p;
    p.jx = warp_clamp(U >> 17, t.crop_w, &inx);
    p.jy = warp_clamp(V >> 17, t.crop_h, &iny);
    p.keep = clamp || (inx && iny);
    return p;
}

// the BILINEAR taps of (U, V): the sample offsets of the two rows and the two pixels, all four clamped into the crop, the
// keep flag of each tap (clamp: as for warp_pick), the Q14 weights of both axes
struct WarpTaps {
    uint64_t r0, r1, c0, c1;
    uint32_t w0x, w1x, w0y, w1y;
    bool k00, k01, k10, k11;
    // channel c at precision P: the horizontal pass rounded to 16 bits, the vertical pass into 30; bd: its border sample
    template <uint32_t P, class Sample>
    DEV_MEMBER_INLINE uint32_t value(const Sample *s, uint32_t c, uint32_t bd) const
    {
        uint32_t s00 = s[r0 + c0 + c], s01 = s[r0 + c1 + c], s10 = s[r1 + c0 + c], s11 = s[r1 + c1 + c];
        if (!k00) s00 = bd;
        if (!k01) s01 = bd;
        if (!k10) s10 = bd;
        if (!k11) s11 = bd;
        const uint32_t h0 = (w0x * s00 + w1x * s01 + (1u << (P - 3u))) >> (P - 2u);
        const uint32_t h1 = (w0x * s10 + w1x * s11 + (1u << (P - 3u))) >> (P - 2u);
        return w0y * h0 + w1y * h1;
    }
};
template <class Task>
DEV_INLINE WarpTaps warp_taps(const Task &t, bool clamp, int64_t U, int64_t V)
{
    const int64_t tu = U - 65536, tv = V - 65536;
    const int64_t ix = tu >> 17, iy = tv >> 17;
    bool ix0, ix1, iy0, iy1;
    const uint32_t x0 = warp_clamp(ix, t.crop_w, &ix0), x1 = warp_clamp(ix + 1, t.crop_w, &ix1);
    const uint32_t y0 = warp_clamp(iy, t.crop_h, &iy0), y1 = warp_clamp(iy + 1, t.crop_h, &iy1);
    WarpTaps q;
    q.w1x = ((uint32_t)(tu & 0x1FFFF) + 4u) >> 3; q.w0x = 16384u - q.w1x;
    q.w1y = ((uint32_t)(tv & 0x1FFFF) + 4u) >> 3; q.w0y = 16384u - q.w1y;
    q.k00 = clamp || (ix0 && iy0); q.k01 = clamp || (ix1 && iy0); q.k10 = clamp || (ix0 && iy1); q.k11 = clamp || (ix1 && iy1);
    q.r0 = (uint64_t)y0 * t.src_pitch; q.r1 = (uint64_t)y1 * t.src_pitch;
    q.c0 = (uint64_t)x0 * t.channels; q.c1 = (uint64_t)x1 * t.channels;
    return q;
}

// the rows of one task at source precision P, its pixels and their (U, V) from the map
template <uint32_t P, class Map, class Task>
DEV_INLINE void warp_rows(const Map &map, const Task &t, const Task *__restrict__ tg, const uint8_t *__restrict__ src,
                          uint8_t *__restrict__ out, uint32_t tid)
{
    typedef typename RszSample<P>::sample_t sample_t;
    const sample_t *s = reinterpret_cast<const sample_t *>(src + t.src_off);
    uint8_t *o = out + t.out_off;
    const uint32_t ch = t.channels;
    const bool clamp = t.border_mode == WARP_BORDER_CLAMP, nearest = t.filter == WARP_FILTER_NEAREST;
    warp_walk(map, t, tid, [&](uint32_t X, uint32_t Y, int64_t U, int64_t V) {
        const uint64_t el = (uint64_t)X * t.out_sx + (uint64_t)Y * t.out_sy;
        if (nearest) {
            const WarpPick p = warp_pick(t, clamp, U, V);
            const uint64_t at = (uint64_t)p.jy * t.src_pitch + (uint64_t)p.jx * ch;
            for (uint32_t c = 0; c < ch; c++) {
                uint32_t v = s[at + c];
                if (!p.keep) v = tg->border[c];
                rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, v << (30u - P));
            }
        } else {
            const WarpTaps q = warp_taps(t, clamp, U, V);
            for (uint32_t c = 0; c < ch; c++)
                rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, q.value<P>(s, c, tg->border[c]));
        }
    });
}

// the image kind: the task loop of debig_png_warp_kernel, _persp_kernel and _elastic_kernel
template <class Task, class Map>
DEV_INLINE void warp_image_tasks(Map map, const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const Task *__restrict__ tasks,
                                 uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const Task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || t.channels == 0u || t.channels > 4u ||
            (t.bits != 8u && t.bits != 16u) || t.dtype > 3u || (t.filter != WARP_FILTER_BILINEAR && t.filter != WARP_FILTER_NEAREST) ||
            t.border_mode > WARP_BORDER_CLAMP || !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) ||
            (t.src_off & ((uint32_t)t.bits / 8u - 1u)) || !map.task_ok(t))
            continue;
        if (!map.hold(t, tid)) continue;
        if (t.bits == 8u) warp_rows<8u>(map, t, &tasks[ti], src, out, tid);
        else warp_rows<16u>(map, t, &tasks[ti], src, out, tid);
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const debig_png_warp_task *__restrict__ tasks,
                      uint32_t n_tasks)
{
    warp_image_tasks(WarpAffine(), src, out, tasks, n_tasks);
}

// ---- the same warp of raw labels: nearest only, the picks of the image kernel's NEAREST filter ---------------------------------

// the rows of one task: elements of ES bytes, source labels of SB bytes
template <uint32_t ES, uint32_t SB, class Map, class Task>
DEV_INLINE void warp_label_rows(const Map &map, const int32_t *lut, const Task &t, const uint8_t *__restrict__ src,
                                uint8_t *__restrict__ out, uint32_t tid)
{
    const uint8_t *s0 = src + t.src_off;
    const bool clamp = t.border_mode == WARP_BORDER_CLAMP;
    warp_walk(map, t, tid, [&](uint32_t X, uint32_t Y, int64_t U, int64_t V) {
        const WarpPick p = warp_pick(t, clamp, U, V);
        const uint64_t at = (uint64_t)p.jy * t.src_pitch + p.jx;
        uint32_t v = SB == 1u ? (uint32_t)s0[at] : (uint32_t)reinterpret_cast<const uint16_t *>(s0)[at];
        if (lut) v = (uint32_t)lut[v & 255u];
        if (!p.keep) v = (uint32_t)t.border_label;
        lbl_store1<ES>(out + t.out_off + ((uint64_t)Y * t.out_w + X) * ES, v);
    });
}

// the label kind: the task loop of debig_png_label_warp_kernel, _label_persp_kernel and _label_elastic_kernel; lds_lut: 256 words
// of LDS that the kernel owns
template <class Task, class Map>
DEV_INLINE void warp_label_tasks(Map map, int32_t *lds_lut, const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                                 const Task *__restrict__ tasks, const int32_t *__restrict__ lut, uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    if (lut) lds_lut[tid & 255u] = lut[tid & 255u];
    __syncthreads();
    const int32_t *L = lut ? lds_lut : nullptr;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const Task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || (t.src_bytes != 1u && t.src_bytes != 2u) ||
            t.dtype > 3u || (t.dtype == 0u && t.src_bytes == 2u) || (lut && t.src_bytes == 2u) || t.border_mode > WARP_BORDER_CLAMP ||
            !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) || (t.src_off & (t.src_bytes - 1u)) || !map.task_ok(t))
            continue;
        if (!map.hold(t, tid)) continue;
        if (t.src_bytes == 1u) {
            if (t.dtype == 0u) warp_label_rows<1u, 1u>(map, L, t, src, out, tid);
            else if (t.dtype == 1u) warp_label_rows<2u, 1u>(map, L, t, src, out, tid);
            else if (t.dtype == 2u) warp_label_rows<4u, 1u>(map, L, t, src, out, tid);
            else warp_label_rows<8u, 1u>(map, L, t, src, out, tid);
        } else {
            if (t.dtype == 1u) warp_label_rows<2u, 2u>(map, L, t, src, out, tid);
            else if (t.dtype == 2u) warp_label_rows<4u, 2u>(map, L, t, src, out, tid);
            else warp_label_rows<8u, 2u>(map, L, t, src, out, tid);
        }
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_label_warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                            const debig_png_label_warp_task *__restrict__ tasks, const int32_t *__restrict__ lut, uint32_t n_tasks)
{
    __shared__ int32_t lds_lut[256];
    warp_label_tasks(WarpAffine(), lds_lut, src, out, tasks, lut, n_tasks);
}
