// png_color_kernel.inc -- one 3 x 4 colour matrix per image (brightness, contrast, saturation, hue, channel order, negative) inside
// the resize and the warp of decoded PNG pixels into one dense tensor
// (include/decode_png.h: debig_png_decode_batch_tensor_color, debig_png_decode_batch_tensor_warp_color; include/debig_hip.h:
// debig_hip_png_resize_color_batch, debig_hip_png_warp_color_batch).
//
// The arithmetic is fixed by decode_png.h: the matrix quantised once on the host (k: Q16 int32, |k| <= 2^20; o: int64 in units of
// v), applied to the three colour values v_j the filter delivers (the sample times 2^(30 - P), below 2^30) in 64-bit integers:
//     acc_c = k_c0 v_0 + k_c1 v_1 + k_c2 v_2   (|acc| < 2^52),   v'_c = clamp(((acc_c + 32768) >> 16) + o_c, 0, Vmax),
// then the ONE conversion of the resize kernels (rsz_cubic_store).  A fourth channel (alpha) is not mixed.
//
// The matrix is uniform over a task: it is one 64-byte record per image in the weights buffer, found through the task's
// color_off and read once per task at a uniform address (scalar loads); it is passed on by value and indexed by unrolled
// constants only, so nothing goes to scratch.
//   - debig_png_resize_color_kernel: the tile, the axis tables, the LDS budget and pass 1 are those of debig_png_resize_kernel
//     (rsz_tile_begin, rsz_sample_pass1; the channels are independent there: items per SAMPLE).  Pass 2 takes an output PIXEL
//     per item, lanes along x: the lane sums its 3 or 4 channels down the Hq rows (halfwords that lie side by side in LDS),
//     mixes, converts and stores that many adjacent elements (HWC) or one element in each plane row, adjacent to its neighbour
//     lanes' (CHW): the store shapes of the alpha kernel.
//   - debig_png_warp_color_kernel: the walk and the picks of png_warp_kernel.inc (warp_walk, warp_pick, warp_taps) with the
//     per-channel store of warp_rows replaced by collect, mix, store; its task loop (warp_color_tasks) is a template over the
//     task and the map, which png_persp_kernel.inc and png_elastic_kernel.inc instantiate again.  Picks, border rule and clamps are the warp kernel's; a
//     CONSTANT border sample is mixed like any other sample.
// A task that breaks a bound -- those of the kernels they extend, channels other than 3 / 4, a color_off that is no multiple of
// 8, a record beyond the quantiser's limits -- is skipped (never indexed out of range).  No atomics, no scratch, nothing shared
// between workgroups; plain vector stores only.
// This file holds the mix and the two bodies that apply it; it repeats no step of the kernels it extends.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_resize_kernel.inc and png_warp_kernel.inc in
// front of it.

#define COLOR_K_MAX (1 << 20) // |m| <= 16 in Q16

// the quantiser's limits on a record at precision P: they keep |acc| below 2^52 and the sum with o far inside int64
DEV_INLINE bool color_rec_ok(const debig_png_color_rec &r, uint32_t P)
{
    const int64_t omax = (int64_t)16 * (int64_t)(((1u << P) - 1u) << (30u - P));
    bool ok = true;
RSZ_UNROLL
    for (uint32_t j = 0; j < 9u; j++) ok = ok && r.k[j] >= -COLOR_K_MAX && r.k[j] <= COLOR_K_MAX;
RSZ_UNROLL
    for (uint32_t c = 0; c < 3u; c++) ok = ok && r.o[c] >= -omax && r.o[c] <= omax;
    return ok;
}

// the mix: three v (below 2^30) -> three v' inside [0, vmax]; 64-bit integers, the shift arithmetic, ONE clamp at the end
DEV_INLINE void color_mix(const debig_png_color_rec &r, uint32_t vmax, const uint32_t *v, uint32_t *m)
{
RSZ_UNROLL
    for (uint32_t c = 0; c < 3u; c++) {
        const int64_t acc = (int64_t)r.k[3u * c] * (int64_t)(int32_t)v[0] + (int64_t)r.k[3u * c + 1u] * (int64_t)(int32_t)v[1] +
                            (int64_t)r.k[3u * c + 2u] * (int64_t)(int32_t)v[2];
        const int64_t q = ((acc + 32768) >> 16) + r.o[c];
        m[c] = (uint32_t)(q < 0 ? 0 : q > (int64_t)vmax ? (int64_t)vmax : q);
    }
}

// pass 2 of one tile for source precision P: an output pixel per item.  The channel count sc (3 or 4) is a run-time value, uniform
// over the task: the three colours are unrolled, the alpha of RGBA sits behind a uniform branch (one instantiation per P instead of
// one per (P, sc) keeps the scalar registers of the kernel within what there is)
template <uint32_t P>
DEV_INLINE void rsz_color_pass2(const RszLds &lds, const debig_png_resize_color_task &t,
                                const debig_png_resize_color_task *__restrict__ tg, const debig_png_color_rec &cr,
                                uint8_t *__restrict__ out, const RszAxes &ax, uint32_t tid)
{
    constexpr uint32_t VMAX = ((1u << P) - 1u) << (30u - P);
    const uint32_t tw = t.tile_w, sc = t.channels, twc = tw * sc, n2 = t.tile_h * tw;
    const bool alpha = sc == 4u;
    uint8_t *o = out + t.out_off;
    for (uint32_t i = tid; i < n2; i += RSZ_THREADS) {
        const uint32_t yy = i / tw, x = i - yy * tw;
        const uint32_t Y = t.tile_y + yy, fy = ax.ty[2u + 2u * Y], cnt = ax.ty[3u + 2u * Y];
        const int16_t *w = ax.wyg + (uint64_t)Y * ax.mty;
        const uint16_t *h = &lds.hq[(fy - t.src_y0) * twc + x * sc];
        uint32_t v[3], m[3], va = 0u;
RSZ_UNROLL
        for (uint32_t c = 0; c < 3u; c++) v[c] = 0u;
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t wk = (uint32_t)w[k];
RSZ_UNROLL
            for (uint32_t c = 0; c < 3u; c++) v[c] += wk * h[k * twc + c];
            if (alpha) va += wk * h[k * twc + 3u];
        }
        color_mix(cr, VMAX, v, m);
        const uint64_t el = (uint64_t)(t.tile_x + x) * t.out_sx + (uint64_t)Y * t.out_sy;
RSZ_UNROLL
        for (uint32_t c = 0; c < 3u; c++) rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, m[c]);
        if (alpha) rsz_cubic_store(t.dtype, P, tg->a[3], tg->b[3], o, el + (uint64_t)3u * t.out_sc, va);
    }
}

__global__ void __launch_bounds__(RSZ_THREADS)
debig_png_resize_color_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                              const debig_png_resize_color_task *__restrict__ tasks, const uint8_t *__restrict__ weights,
                              uint32_t n_tasks)
{
    __shared__ RszLds lds;
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_resize_color_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if ((t.channels != 3u && t.channels != 4u) || (t.bits != 8u && t.bits != 16u) || t.dtype > 3u || (t.color_off & 7u)) continue;
        debig_png_color_rec cr;
        RszAxes ax;
        if (!rsz_tile_begin(lds, t, weights, tid, ax, [&] {
                cr = *reinterpret_cast<const debig_png_color_rec *>(weights + t.color_off);
                return color_rec_ok(cr, t.bits);
            }))
            continue;
        rsz_sample_pass1(lds, t, src, ax.mtx, tid);
        __syncthreads();
        // ---- pass 2: v_c = sum_k wy[Y][k] * Hq[fy[Y] + k][x][c] of the pixel's channels, the mix, then the one conversion
        if (t.bits == 8u) rsz_color_pass2<8u>(lds, t, &tasks[ti], cr, out, ax, tid);
        else rsz_color_pass2<16u>(lds, t, &tasks[ti], cr, out, ax, tid);
    }
}

// ---- the warp with the matrix ------------------------------------------------------------------------------------------------------

// the rows of one task at source precision P: the walk and the picks of warp_rows (png_warp_kernel.inc), the pixel's channels
// collected, mixed and stored; the channel count sc is a run-time value as in rsz_color_pass2
template <uint32_t P, class Map, class Task>
DEV_INLINE void warp_color_rows(const Map &map, const Task &t, const Task *__restrict__ tg, const debig_png_color_rec &cr,
                                const uint8_t *__restrict__ src, uint8_t *__restrict__ out, uint32_t tid)
{
    typedef typename RszSample<P>::sample_t sample_t;
    constexpr uint32_t VMAX = ((1u << P) - 1u) << (30u - P);
    const sample_t *s = reinterpret_cast<const sample_t *>(src + t.src_off);
    uint8_t *o = out + t.out_off;
    const uint32_t sc = t.channels;
    const bool alpha = sc == 4u;
    const bool clamp = t.border_mode == WARP_BORDER_CLAMP, nearest = t.filter == WARP_FILTER_NEAREST;
    warp_walk(map, t, tid, [&](uint32_t X, uint32_t Y, int64_t U, int64_t V) {
        const uint64_t el = (uint64_t)X * t.out_sx + (uint64_t)Y * t.out_sy;
        uint32_t v[3], m[3], va = 0u;
        if (nearest) {
            const WarpPick p = warp_pick(t, clamp, U, V);
            const uint64_t at = (uint64_t)p.jy * t.src_pitch + (uint64_t)p.jx * sc;
RSZ_UNROLL
            for (uint32_t c = 0; c < 3u; c++) {
                uint32_t sv = s[at + c];
                if (!p.keep) sv = tg->border[c];
                v[c] = sv << (30u - P);
            }
            if (alpha) {
                uint32_t sv = s[at + 3u];
                if (!p.keep) sv = tg->border[3];
                va = sv << (30u - P);
            }
        } else {
            const WarpTaps q = warp_taps(t, clamp, U, V);
RSZ_UNROLL
            for (uint32_t c = 0; c < 3u; c++) v[c] = q.value<P>(s, c, tg->border[c]);
            if (alpha) va = q.value<P>(s, 3u, tg->border[3]);
        }
        color_mix(cr, VMAX, v, m);
RSZ_UNROLL
        for (uint32_t c = 0; c < 3u; c++) rsz_cubic_store(t.dtype, P, tg->a[c], tg->b[c], o, el + (uint64_t)c * t.out_sc, m[c]);
        if (alpha) rsz_cubic_store(t.dtype, P, tg->a[3], tg->b[3], o, el + (uint64_t)3u * t.out_sc, va);
    });
}

// the colour kind: the task loop of debig_png_warp_color_kernel, _persp_color_kernel and _elastic_color_kernel.  The record is
// read and checked in front of the map's hold step
template <class Task, class Map>
DEV_INLINE void warp_color_tasks(Map map, const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const Task *__restrict__ tasks,
                                 const uint8_t *__restrict__ weights, uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const Task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || (t.channels != 3u && t.channels != 4u) ||
            (t.bits != 8u && t.bits != 16u) || t.dtype > 3u || (t.filter != WARP_FILTER_BILINEAR && t.filter != WARP_FILTER_NEAREST) ||
            t.border_mode > WARP_BORDER_CLAMP || !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) ||
            (t.src_off & ((uint32_t)t.bits / 8u - 1u)) || (t.color_off & 7u) || !map.task_ok(t))
            continue;
        const debig_png_color_rec cr = *reinterpret_cast<const debig_png_color_rec *>(weights + t.color_off);
        if (!color_rec_ok(cr, t.bits)) continue;
        if (!map.hold(t, tid)) continue;
        if (t.bits == 8u) warp_color_rows<8u>(map, t, &tasks[ti], cr, src, out, tid);
        else warp_color_rows<16u>(map, t, &tasks[ti], cr, src, out, tid);
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_warp_color_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                            const debig_png_warp_color_task *__restrict__ tasks, const uint8_t *__restrict__ weights, uint32_t n_tasks)
{
    warp_color_tasks(WarpAffine(), src, out, tasks, weights, n_tasks);
}
