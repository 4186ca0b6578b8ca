// png_color_label_kernel.inc -- crop + nearest pick + colour pack + colour -> class lookup + widening of decoded RGB8 masks
// into one dense integer tensor (include/decode_png.h: debig_png_decode_batch_color_labels; include/debig_hip.h:
// debig_hip_png_color_label_batch).
//
// The source is what the output-format de-filter left in the arena: interleaved RGB8, three bytes per pixel at ANY alignment.
// Output element (X, Y) of an image is the pixel at sy[Y] * pitch + sx[X] of its crop, packed as key = R | G << 8 | B << 16;
// PACK stores the key, MAP stores values[k] of the key's entry in the image's table, or `missing`, and counts the misses.
// sx and sy are the host-made index tables of the raw-label gather (png_label_kernel.inc) and so is the decomposition:
//   - one TASK is a run of output rows of one image, one workgroup of 256 lanes per task; an ITEM is E adjacent elements of
//     one output row (E = 8, 8, 4, 2 for uint8, uint16, int32, int64), lanes along x and on into the next row of the run;
//     full items go out through spec_store_run (the widest store the address allows), the last item of a row element by
//     element;
//   - a pick is three byte loads (a pixel starts at any byte, and nothing past the crop's last pixel is read);
//   - the TABLE (include/debig_hip.h: debig_png_color_label_task) is open addressing with linear probing, key and value side
//     by side, staged in LDS slot by slot: 8 bytes per slot, at most 4096 slots = 32 KB.  The workgroup stages it when the
//     task's table offset or slot count differs from the one it holds -- once per workgroup when the call has one map;
//   - label maps are blocky: a lane keeps the key, value and hit flag of its previous pick and probes LDS only when the key
//     changes (the lanes of one ds_read then mostly hit one address, a broadcast);
//   - probing stops at the key, at an empty slot, or after `slots` probes: it terminates on any table contents;
//   - misses are counted per lane over the task, summed over the wavefront with shuffles, and ONE atomicAdd per wavefront and
//     task goes to the image's counter.
// A task that breaks a bound is skipped (never indexed out of range); PACK never touches the table or the counters.
// No scratch (every per-item array is indexed by unrolled constants), no inline assembly.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_stage_common.inc and png_label_kernel.inc
// in front of it.

#define CLBL_THREADS 256u

DEV_INLINE uint32_t clbl_slot(uint32_t key, uint32_t slots) { return DEBIG_PNG_CMAP_SLOT(key, slots); }

// the value of `key` in the staged table -> true, or false (not in the map)
DEV_INLINE bool clbl_find(const uint2 *tab, uint32_t slots, uint32_t key, uint32_t &val)
{
    uint32_t s = clbl_slot(key, slots);
    for (uint32_t k = 0; k < slots; k++) {
        const uint2 e = tab[s];
        if (e.x == key) { val = e.y; return true; }
        if (e.x == DEBIG_PNG_CMAP_EMPTY) return false;
        s = (s + 1u) & (slots - 1u);
    }
    return false;
}

// one pick: the packed colour at pixel `el` of the crop, and its element (PACK: the key)
struct ClblPrev { uint32_t key, val, hit; };
template <bool MAP>
DEV_INLINE uint32_t clbl_pick(const uint8_t *__restrict__ s0, uint64_t el, const uint2 *tab, uint32_t slots, uint32_t missing,
                              ClblPrev &pv, uint32_t &misses)
{
    const uint8_t *p = s0 + el * 3u;
    const uint32_t key = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    if (!MAP) return key;
    if (key != pv.key) {
        uint32_t v = missing;
        pv.hit = clbl_find(tab, slots, key, v) ? 1u : 0u;
        pv.key = key;
        pv.val = v;
    }
    misses += 1u - pv.hit;
    return pv.val;
}

// the rows of one task: the row body of the raw-label gather (lbl_gather_rows) with the colour pick -> the lane's misses
template <uint32_t ES, uint32_t E, bool MAP>
DEV_INLINE uint32_t clbl_rows(const uint2 *tab, const debig_png_color_label_task &t, const uint8_t *__restrict__ src,
                              uint8_t *__restrict__ out, const uint32_t *__restrict__ sx, const uint32_t *__restrict__ sy, uint32_t tid)
{
    const uint8_t *s0 = src + t.src_off;
    const uint32_t missing = (uint32_t)t.missing;
    uint32_t misses = 0u;
    ClblPrev pv;
    pv.key = DEBIG_PNG_CMAP_EMPTY; pv.val = missing; pv.hit = 0u; /* no 24-bit key equals it */
    lbl_gather_rows<ES, E>(t, out, sx, sy, tid,
                           [&](uint64_t el) -> uint32_t { return clbl_pick<MAP>(s0, el, tab, t.map_slots, missing, pv, misses); });
    return misses;
}

// ---- what the two colour-label kernels share (this file, png_color_label_warp_kernel.inc) ---------------------------------------

// the table a workgroup holds in LDS: staged when the task's table offset or slot count differs from the one held
struct ClblHeld {
    uint64_t off;   /* ~0: none yet */
    uint32_t slots;
};
template <class Task>
DEV_INLINE void clbl_hold_map(uint2 *lds_map, ClblHeld &held, const Task &t, const uint8_t *__restrict__ tables, uint32_t tid)
{
    if (t.map_off == held.off && t.map_slots == held.slots) return;
    __syncthreads(); /* nobody still probes the table that goes */
    const uint2 *gt = reinterpret_cast<const uint2 *>(tables + t.map_off);
    for (uint32_t k = tid; k < t.map_slots; k += CLBL_THREADS) lds_map[k] = gt[k];
    __syncthreads();
    held.off = t.map_off;
    held.slots = t.map_slots;
}

// the wavefront's misses of one task -> ONE atomicAdd; every lane must be here (the task loop is uniform)
DEV_INLINE void clbl_add_misses(uint32_t *__restrict__ counter, uint32_t m, uint32_t tid)
{
DEV_UNROLL
    for (uint32_t d = 32u; d >= 1u; d >>= 1) m += __shfl_xor(m, (int)d);
    if ((tid & 63u) == 0u && m != 0u) atomicAdd(counter, m);
}

__global__ void __launch_bounds__(CLBL_THREADS)
debig_png_color_label_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                             const debig_png_color_label_task *__restrict__ tasks, const uint8_t *__restrict__ tables,
                             uint32_t *__restrict__ unmatched, uint32_t n_tasks)
{
    __shared__ uint2 lds_map[DEBIG_PNG_CMAP_MAX_SLOTS]; /* (key, value) per slot */
    const uint2 *tab = lds_map;
    const uint32_t tid = threadIdx.x;
    ClblHeld held = { ~(uint64_t)0, 0u };
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_color_label_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (t.out_w == 0u || t.out_w > 16384u || t.out_h > 16384u || t.rows == 0u || t.row0 >= t.out_h || t.rows > t.out_h - t.row0 ||
            t.dtype > 3u || t.mode > 1u || ((t.sx_off | t.sy_off) & 15u))
            continue;
        if (t.mode == 0u ? t.dtype < 2u
                         : (t.map_slots < 2u || t.map_slots > DEBIG_PNG_CMAP_MAX_SLOTS || (t.map_slots & (t.map_slots - 1u)) ||
                            (t.map_off & 15u) || !unmatched))
            continue;
        const uint32_t *sx = reinterpret_cast<const uint32_t *>(tables + t.sx_off);
        const uint32_t *sy = reinterpret_cast<const uint32_t *>(tables + t.sy_off);
        if (t.mode == 0u) {
            if (t.dtype == 2u) clbl_rows<4u, 4u, false>(tab, t, src, out, sx, sy, tid);
            else clbl_rows<8u, 2u, false>(tab, t, src, out, sx, sy, tid);
            continue;
        }
        clbl_hold_map(lds_map, held, t, tables, tid);
        uint32_t m;
        if (t.dtype == 0u) m = clbl_rows<1u, 8u, true>(tab, t, src, out, sx, sy, tid);
        else if (t.dtype == 1u) m = clbl_rows<2u, 8u, true>(tab, t, src, out, sx, sy, tid);
        else if (t.dtype == 2u) m = clbl_rows<4u, 4u, true>(tab, t, src, out, sx, sy, tid);
        else m = clbl_rows<8u, 2u, true>(tab, t, src, out, sx, sy, tid);
        clbl_add_misses(&unmatched[t.image], m, tid);
    }
}
