// png_label_stats_kernel.inc -- per-id pixel counts and bounding boxes of a dense label tensor (include/decode_png.h:
// debig_png_label_stats, which has the rule; include/debig_hip.h: debig_hip_png_label_stats_batch, the raw record and the task).
//
// One TASK is a run of whole rows of one image of the dense (N, H, W) tensor, so a flat range of rows x out_w elements; one
// workgroup of 256 lanes per task.
//   - the lanes read the range in items of 16 bytes at 16-byte aligned addresses (uint4: 16 / 8 / 4 / 2 elements), the elements
//     in front of the first and behind the last item one by one (at most 15 each).  Row and column of a lane's first item come
//     from one division, those of the next (256 items on) from an add and a compare; inside an item the column steps with the
//     element and wraps into the next row where the item crosses a row end;
//   - the key of an element is its value where that is below n_ids, else n_ids ("other": negative values, values of n_ids and
//     above; an int64 whose upper word is not zero is never below n_ids);
//   - label maps are blocky, so a lane carries ONE open record in registers -- key, count, the x extremes, the first and the last
//     row -- and writes it to LDS only when the key changes and at the end of the task.  An item of equal elements inside one row
//     (the common item) is taken whole: one compare chain, then count += its elements;
//   - the image's table is in LDS, structure of arrays with a stride of 1025 words, so the five fields of one id lie on five
//     different banks: count by atomicAdd, max x + 1, max y + 1, out_w - min x and out_h - min y by atomicMax
//     (5 x 1025 x 4 B = 20,500 B).  The workgroup keeps the table across consecutive tasks of one image (same stat_off and n_ids);
//   - when the image changes, and behind its last task, the workgroup flushes: for the entries with a count, one device-scope
//     atomicAdd / atomicMax per field into the image's raw records, whose results are not used; the lane that flushes an entry
//     clears it.  Integer adds and maxima commute: the records are exact whatever the grid and the order.
// A task that breaks a bound is skipped (never indexed out of range).  Nothing waits on another workgroup.  No scratch, no inline
// assembly, plain vector loads.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc and png_stage_common.inc in
// front of it.

#define LST_THREADS 256u
#define LST_STRIDE (DEBIG_PNG_LABEL_STATS_MAX_IDS + 1u) /* words between two fields of one id */

DEV_INLINE bool lst_task_ok(const debig_png_label_stats_task &t, const uint8_t *labels, const uint8_t *stats)
{
    if (t.dtype > 3u || t.n_ids == 0u || t.n_ids > DEBIG_PNG_LABEL_STATS_MAX_IDS) return false;
    // (a run of any length: this kernel has no element budget)
    if (!stage_dim_ok(t.out_w, t.out_h) || !stage_rows_ok(t.out_h, t.row0, t.rows)) return false;
    return stage_addr_ok(stats, t.stat_off, 3u) && stage_addr_ok(labels, t.label_off, (1u << t.dtype) - 1u);
}

// the open record of a lane: n elements of key id (n 0: none) in columns x_lo .. x_hi of rows y_lo .. y_hi
struct LstOpen { uint32_t id, n, x_lo, x_hi, y_lo, y_hi; };

DEV_INLINE void lst_close(uint32_t *tab, const LstOpen &o, uint32_t w, uint32_t h)
{
    if (o.n == 0u) return;
    atomicAdd(&tab[o.id], o.n);
    atomicMax(&tab[LST_STRIDE + o.id], o.x_hi + 1u);
    atomicMax(&tab[2u * LST_STRIDE + o.id], o.y_hi + 1u);
    atomicMax(&tab[3u * LST_STRIDE + o.id], w - o.x_lo);
    atomicMax(&tab[4u * LST_STRIDE + o.id], h - o.y_lo);
}

// cnt elements of value v (0xffffffff: outside every id range) at columns x .. x + cnt - 1 of row y; a lane's rows never decrease
DEV_INLINE void lst_take(uint32_t *tab, LstOpen &o, uint32_t v, uint32_t x, uint32_t y, uint32_t cnt, const debig_png_label_stats_task &t)
{
    const uint32_t key = v < t.n_ids ? v : t.n_ids;
    if (key != o.id || o.n == 0u) {
        lst_close(tab, o, t.out_w, t.out_h);
        o.id = key; o.n = 0u; o.x_lo = x; o.x_hi = x; o.y_lo = y;
    }
    o.n += cnt;
    o.x_lo = x < o.x_lo ? x : o.x_lo;
    o.x_hi = x + cnt - 1u > o.x_hi ? x + cnt - 1u : o.x_hi;
    o.y_hi = y;
}

// are the 16 / ES elements of the item equal?
template <uint32_t ES>
DEV_INLINE bool lst_flat(const uint32_t (&w)[4])
{
    if (ES == 8u) return w[0] == w[2] && w[1] == w[3];
    const uint32_t pat = ES == 1u ? (w[0] & 255u) * 0x01010101u : ES == 2u ? (w[0] & 65535u) * 0x00010001u : w[0];
    return w[0] == pat && w[1] == pat && w[2] == pat && w[3] == pat;
}

// the elements of one task into the table; ES: bytes of an element
template <uint32_t ES>
DEV_INLINE void lst_run(uint32_t *tab, const uint8_t *__restrict__ p, const debig_png_label_stats_task &t, uint32_t tid)
{
    constexpr uint32_t EPI = 16u / ES; /* elements per item */
    const uint32_t W = t.out_w, n_el = t.rows * W; /* <= 2^28 */
    uint32_t head = ((uint32_t)(16u - ((uintptr_t)p & 15u)) & 15u) / ES;
    if (head > n_el) head = n_el;
    const uint32_t items = (n_el - head) / EPI, tail0 = head + items * EPI;
    LstOpen o = {0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    if (tid < head) lst_take(tab, o, lbl_key(lbl_load<ES>(p + (uint64_t)tid * ES)), tid % W, t.row0 + tid / W, 1u, t);
    if (tid < items) {
        const uint32_t e0 = head + tid * EPI;
        StageWalk at(e0, W, LST_THREADS * EPI);
        for (uint32_t u = tid; u < items; u += LST_THREADS) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p + (uint64_t)(head + u * EPI) * ES);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            if (at.x + EPI <= W && lst_flat<ES>(w)) {
                lst_take(tab, o, lbl_key(lbl_item_get<ES>(w, 0u)), at.x, t.row0 + at.r, EPI, t);
            } else {
                uint32_t x = at.x, y = t.row0 + at.r;
DEV_UNROLL
                for (uint32_t j = 0; j < EPI; j++) {
                    lst_take(tab, o, lbl_key(lbl_item_get<ES>(w, j)), x, y, 1u, t);
                    if (++x == W) { x = 0u; y++; }
                }
            }
            at.next();
        }
    }
    if (tid >= 16u && tid - 16u < n_el - tail0) { /* (other lanes than the head's; their items lie in front of the tail) */
        const uint32_t i = tail0 + tid - 16u;
        lst_take(tab, o, lbl_key(lbl_load<ES>(p + (uint64_t)i * ES)), i % W, t.row0 + i / W, 1u, t);
    }
    lst_close(tab, o, W, t.out_h);
}

// the table's entries 0 .. n_ids into the raw records at g, cleared as they go (between two barriers of the caller)
DEV_INLINE void lst_flush(uint32_t *tab, uint32_t *g, uint32_t n_ids, uint32_t tid)
{
    for (uint32_t k = tid; k <= n_ids; k += LST_THREADS) {
        const uint32_t c = tab[k];
        if (c == 0u) continue; /* (an entry without a count has no extremes either) */
        atomicAdd(&g[5u * k], c);
DEV_UNROLL
        for (uint32_t f = 1u; f < 5u; f++) atomicMax(&g[5u * k + f], tab[f * LST_STRIDE + k]);
DEV_UNROLL
        for (uint32_t f = 0u; f < 5u; f++) tab[f * LST_STRIDE + k] = 0u;
    }
}

__global__ void __launch_bounds__(LST_THREADS)
debig_png_label_stats_kernel(const uint8_t *__restrict__ labels, uint8_t *__restrict__ stats,
                             const debig_png_label_stats_task *__restrict__ tasks, uint32_t n_tasks)
{
    __shared__ uint32_t lds_tab[5u * LST_STRIDE]; /* [field][id] */
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < 5u * LST_STRIDE; k += LST_THREADS) lds_tab[k] = 0u;
    __syncthreads();
    uint64_t held_off = 0u; /* the image whose table is in LDS */
    uint32_t held_n = 0u;   /* 0: none yet */
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_stats_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!lst_task_ok(t, labels, stats)) continue;
        if (held_n != 0u && (t.stat_off != held_off || t.n_ids != held_n)) {
            __syncthreads(); /* every lane has closed its record of the image that goes */
            lst_flush(lds_tab, reinterpret_cast<uint32_t *>(stats + held_off), held_n, tid);
            __syncthreads();
        }
        held_off = t.stat_off;
        held_n = t.n_ids;
        const uint8_t *p = labels + t.label_off;
        if (t.dtype == 0u) lst_run<1u>(lds_tab, p, t, tid);
        else if (t.dtype == 1u) lst_run<2u>(lds_tab, p, t, tid);
        else if (t.dtype == 2u) lst_run<4u>(lds_tab, p, t, tid);
        else lst_run<8u>(lds_tab, p, t, tid);
    }
    if (held_n != 0u) {
        __syncthreads();
        lst_flush(lds_tab, reinterpret_cast<uint32_t *>(stats + held_off), held_n, tid);
    }
}
