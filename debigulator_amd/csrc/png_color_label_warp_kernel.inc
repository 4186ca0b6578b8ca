// png_color_label_warp_kernel.inc -- crop + affine warp + colour pack + colour -> class lookup + widening of decoded RGB8 masks
// into one dense integer tensor (include/decode_png.h: debig_png_decode_batch_color_labels_warp; include/debig_hip.h:
// debig_hip_png_color_label_warp_batch).
//
// The colour-label gather (png_color_label_kernel.inc) with its sx / sy grid replaced by the pick of the label warp
// (png_warp_kernel.inc: warp_walk, warp_pick): the same six int64 in the task, the same U, V in Q17, (jx, jy) = (U >> 17, V >> 17).
//   - one TASK is a run of output rows of one image, one workgroup of 256 lanes per task; an ITEM is one output element, the
//     lanes run along X and on into the next row of the run (the decomposition of debig_png_label_warp_kernel);
//   - both indices are clamped into the crop BEFORE they address memory, whatever the border mode; then three byte loads at
//     src_off + (jy * src_pitch + jx) * 3: a pixel starts at any byte, and nothing outside the crop is read.  Under CONSTANT
//     the looked-up value is replaced by border_label by a select: no branch diverges on the position;
//   - the TABLE, its slot function and the probe are those of the gather (clbl_find), staged in LDS when the task's table
//     offset or slot count differs from the one held, between the same two barriers (clbl_hold_map);
//   - no previous-key reuse: a lane's consecutive picks lie 256 output elements apart (other rows, other source pixels), and
//     a wavefront skips its probe loop only when all 64 lanes repeat their key; what that could save is one ds_read_b64 and
//     a multiply per element next to three dependent global byte loads (DESIGN.md has the reasoning);
//   - misses are counted per lane over the task -- an element that took border_label is none --, summed over the wavefront
//     with six shuffles, and ONE atomicAdd per wavefront and task goes to the image's counter (clbl_add_misses).
// The task loop (clbl_warp_tasks) is a template over the task and the map (png_warp_kernel.inc has the scheme); this file's
// kernel is its affine instance, png_persp_kernel.inc and png_elastic_kernel.inc have the other two.
// A task that breaks a bound is skipped (never indexed out of range); PACK never touches the table or the counters.
// No scratch, no inline assembly, plain vector stores only.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_stage_common.inc,
// png_color_label_kernel.inc and png_warp_kernel.inc in front of it.

// the rows of one task: elements of ES bytes -> the lane's misses
template <uint32_t ES, bool MAP, class Map, class Task>
DEV_INLINE uint32_t clbl_warp_rows(const Map &map, const uint2 *tab, const Task &t, const uint8_t *__restrict__ src,
                                   uint8_t *__restrict__ out, uint32_t tid)
{
    const uint8_t *s0 = src + t.src_off;
    const uint32_t missing = (uint32_t)t.missing;
    uint32_t misses = 0u;
    const bool clamp = t.border_mode == WARP_BORDER_CLAMP;
    warp_walk(map, t, tid, [&](uint32_t X, uint32_t Y, int64_t U, int64_t V) {
        const WarpPick pk = warp_pick(t, clamp, U, V);
        const uint8_t *p = s0 + ((uint64_t)pk.jy * t.src_pitch + pk.jx) * 3u;
        const uint32_t key = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        uint32_t v = key;
        if (MAP) {
            v = missing;
            const bool hit = clbl_find(tab, t.map_slots, key, v);
            misses += pk.keep && !hit ? 1u : 0u;
        }
        if (!pk.keep) v = (uint32_t)t.border_label;
        lbl_store1<ES>(out + t.out_off + ((uint64_t)Y * t.out_w + X) * ES, v);
    });
    return misses;
}

// the colour-label kind: the task loop of debig_png_color_label_warp_kernel, _persp_kernel and _elastic_kernel; lds_map:
// DEBIG_PNG_CMAP_MAX_SLOTS (key, value) slots of LDS that the kernel owns
template <class Task, class Map>
DEV_INLINE void clbl_warp_tasks(Map map, uint2 *lds_map, const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                                const Task *__restrict__ tasks, const uint8_t *__restrict__ tables, uint32_t *__restrict__ unmatched,
                                uint32_t n_tasks)
{
    const uint2 *tab = lds_map;
    const uint32_t tid = threadIdx.x;
    ClblHeld held = { ~(uint64_t)0, 0u };
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const Task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!warp_sizes_ok(t.out_w, t.out_h, t.row0, t.rows, t.crop_w, t.crop_h) || t.dtype > 3u || t.mode > 1u ||
            t.border_mode > WARP_BORDER_CLAMP || !warp_matrix_ok(t.m[0], t.m[1], t.m[2], t.m[3], t.m[4], t.m[5]) || !map.task_ok(t))
            continue;
        if (t.mode == 0u ? t.dtype < 2u
                         : (t.map_slots < 2u || t.map_slots > DEBIG_PNG_CMAP_MAX_SLOTS || (t.map_slots & (t.map_slots - 1u)) ||
                            (t.map_off & 15u) || !unmatched))
            continue;
        if (!map.hold(t, tid)) continue;
        if (t.mode == 0u) {
            if (t.dtype == 2u) clbl_warp_rows<4u, false>(map, tab, t, src, out, tid);
            else clbl_warp_rows<8u, false>(map, tab, t, src, out, tid);
            continue;
        }
        clbl_hold_map(lds_map, held, t, tables, tid);
        uint32_t m;
        if (t.dtype == 0u) m = clbl_warp_rows<1u, true>(map, tab, t, src, out, tid);
        else if (t.dtype == 1u) m = clbl_warp_rows<2u, true>(map, tab, t, src, out, tid);
        else if (t.dtype == 2u) m = clbl_warp_rows<4u, true>(map, tab, t, src, out, tid);
        else m = clbl_warp_rows<8u, true>(map, tab, t, src, out, tid);
        clbl_add_misses(&unmatched[t.image], m, tid);
    }
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_color_label_warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                                  const debig_png_color_label_warp_task *__restrict__ tasks, const uint8_t *__restrict__ tables,
                                  uint32_t *__restrict__ unmatched, uint32_t n_tasks)
{
    __shared__ uint2 lds_map[DEBIG_PNG_CMAP_MAX_SLOTS]; /* (key, value) per slot */
    clbl_warp_tasks(WarpAffine(), lds_map, src, out, tasks, tables, unmatched, n_tasks);
}
