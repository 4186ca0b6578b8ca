// png_label_distance_kernel.inc -- exact squared Euclidean distance maps of a dense label tensor (include/decode_png.h:
// debig_png_label_distance, which has the rule; include/debig_hip.h: debig_hip_png_label_distance_rows_batch / _cols_batch and the
// two tasks).  D2(x, y) = min over the SITES (x', y') of (x, y) of (x - x')^2 + (y - y')^2, in two launches, each linear in the
// row or column length whatever the data holds:
//
// ROWS (debig_png_label_distance_rows_kernel): one TASK is a run of whole rows of one image, at most 16384 elements, so a flat
// range; one workgroup of 256 lanes.  It writes the G PLANE, one uint16 per element: bits 0 .. 14 the distance along the row to the
// nearest site of the element in that row (0 .. 16383; LDG_NONE: the row has none), bit 15 "differs from the element above"
// (DIFFERS only; never in row 0).  The row distance comes from two segmented scans over the flat range, not from stepping outward:
//   - a FLAG is an element equal to `value` (TO_VALUE), or the first / last element of a same-valued run that does not touch the
//     row's start / end (DIFFERS: the site is the element in front of / behind the run);
//   - the left scan is an inclusive maximum of the key 2 i + 1 of a flagged element i and 2 i of an unflagged row start (a
//     barrier: an even result means "no site to the left in this row"), the right scan an inclusive minimum of 2 i / 2 i + 1 / none;
//   - the range is cut into segments of 64 elements, one per wavefront and step.  Step 1: every segment's maximum / minimum by wave
//     shuffles into LDS.  Step 2: the 256 lanes scan the (at most 256) segment aggregates, shuffles inside a wavefront and a carry
//     through LDS between the four, so every segment knows what comes in from its left and its right.  Step 3: every segment again,
//     an inclusive shuffle scan plus the carry, and the store.  Three barriers per task, whatever the data.
//
// COLS (debig_png_label_distance_cols_kernel): one TASK is a strip of at most 64 adjacent columns of one image, one lane per
// column, one wavefront per task: the 64 lanes read one 128-byte line of the g plane per row.  It never reads the labels.  Each
// lane runs Meijster's two scans over every RUN of its column -- the whole column under TO_VALUE (bit 15 is never set), a maximal
// same-valued run under DIFFERS, seeded with a virtual site of row distance 0 in the row above it and closed with one in the row
// below it where the image has those rows:
//   - forward, a row with a row distance g is the parabola f(u) = (u - s)^2 + g^2; the lower envelope is a stack of (site row s,
//     first row t it serves).  A candidate that beats the top at the top's t pops it; otherwise it is pushed at
//     t = 1 + Sep(top, candidate), Sep(i, u) = floor((u^2 - i^2 + g(u)^2 - g(i)^2) / (2 (u - i))), when that is a row of the image;
//   - backward, from the run's last row up, the top serves the row and is popped at its t.
// THE STACK LIVES IN THE COLUMN'S OWN SLOTS OF THE OUTPUT PLANE (two uint16 in one 4-byte element): the top is in registers, entry
// k below it in the slot of row a + k of a run that starts in row a.  Entry k was pushed by row a + k or a later one and serves rows
// from t >= a + k on, so during the backward scan every live entry lies at or above the row being written, and a run never touches
// another run's rows.  The two virtual sites are never stored: the upper one is entry 0 and is rebuilt from the run's start, the
// lower one is pushed last and stays in registers.  A lane is a flat state machine -- every trip of its loop fetches at most one
// row, tries at most one pop or push, or writes at most one row -- so the trips of a wavefront are bounded by 7 x out_h whatever the
// lanes' runs look like (no loop whose trip count is another lane's run length).
// The cap, NONE and the one conversion (int32 D2, or the float32 nearest to its square root: (float)sqrt((double)d2), see
// decode_png.h) happen at the final store.
// A task that breaks a bound is skipped (never indexed out of range).  Nothing waits on another workgroup.  No scratch, no inline
// assembly, plain vector loads and stores.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc and
// png_stage_common.inc in front of it.

#ifdef DEBIG_EMU
#include <math.h> /* sqrt: the emulator build is plain C++ */
#endif

#define LDR_THREADS 256u
#define LDC_THREADS 64u
#define LDG_NONE 0x7fffu  /* bits 0 .. 14 of a g element: the row has no site for it */
#define LDG_ABOVE 0x8000u /* bit 15: the element differs from the one above it */
#define LDR_NO_KEY 0x7fffffff

DEV_INLINE bool ldr_task_ok(const debig_png_label_distance_rows_task &t, const uint8_t *labels, const uint8_t *g)
{
    if (t.dtype > 3u || t.sites > 1u) return false;
    if (!stage_dim_ok(t.w, t.h) || !stage_rows_ok(t.h, t.row0, t.rows)) return false;
    if (!stage_budget_ok(t.rows, t.w, DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS)) return false;
    return stage_addr_ok(labels, t.label_off, (1u << t.dtype) - 1u) && stage_addr_ok(g, t.g_off, 1u);
}

DEV_INLINE bool ldc_task_ok(const debig_png_label_distance_cols_task &t, const uint8_t *g, const uint8_t *out)
{
    if (t.format > 1u || t.cap > 32767u) return false;
    if (!stage_dim_ok(t.w, t.h)) return false;
    if (t.cols == 0u || t.cols > LDC_THREADS || t.x0 >= t.w || t.cols > t.w - t.x0) return false;
    return stage_addr_ok(g, t.g_off, 1u) && stage_addr_ok(out, t.out_off, 3u);
}

// the two scan keys of element i of the flat range (none: -1 / LDR_NO_KEY) and its "differs from the element above" bit
struct LdrKeys { int32_t left, right; uint32_t above; };

template <uint32_t ES, bool TO_VALUE>
DEV_INLINE LdrKeys ldr_keys(const uint8_t *in, const debig_png_label_distance_rows_task &t, uint32_t i, uint32_t n_el, uint2 want, bool possible)
{
    LdrKeys k = {-1, LDR_NO_KEY, 0u};
    if (i >= n_el) return k;
    const uint32_t W = t.w, r = i / W, x = i - r * W;
    const uint2 v = lbl_load<ES>(in + (uint64_t)i * ES);
    bool fl, fr;
    if (TO_VALUE) {
        fl = fr = possible && lbl_same(v, want);
    } else {
        fl = fr = false;
        if (x > 0u) {
            const uint2 u = lbl_load<ES>(in + (uint64_t)(i - 1u) * ES);
            fl = !lbl_same(u, v);
        }
        if (x + 1u < W) {
            const uint2 u = lbl_load<ES>(in + (uint64_t)(i + 1u) * ES);
            fr = !lbl_same(u, v);
        }
        if (t.row0 + r > 0u) { /* (the row above a task's first row belongs to the image, if not to the task) */
            const uint2 u = lbl_load<ES>(in + ((int64_t)i - (int64_t)W) * (int64_t)ES);
            k.above = !lbl_same(u, v) ? LDG_ABOVE : 0u;
        }
    }
    k.left = fl ? (int32_t)(2u * i + 1u) : x == 0u ? (int32_t)(2u * i) : -1;
    k.right = fr ? (int32_t)(2u * i) : x + 1u == W ? (int32_t)(2u * i + 1u) : LDR_NO_KEY;
    return k;
}

DEV_INLINE int32_t ldr_max(int32_t a, int32_t b) { return a > b ? a : b; }
DEV_INLINE int32_t ldr_min(int32_t a, int32_t b) { return a < b ? a : b; }

// one task; ES: bytes of an element.  lds: [0, 256) the segments' maxima, then what comes in from the left; [256, 512) the minima,
// then what comes in from the right; [512, 516) / [516, 520) the four wavefronts' totals
template <uint32_t ES, bool TO_VALUE>
DEV_INLINE void ldr_run(int32_t *lds, const uint8_t *__restrict__ labels, uint8_t *__restrict__ g, const debig_png_label_distance_rows_task &t,
                        uint32_t tid)
{
    const uint32_t W = t.w, n_el = t.rows * W, n_seg = (n_el + 63u) >> 6; /* n_el <= 16384: at most 256 segments */
    const uint8_t *in = labels + t.label_off + (uint64_t)t.row0 * W * ES;
    uint16_t *gp = reinterpret_cast<uint16_t *>(g + t.g_off) + (uint64_t)t.row0 * W;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    uint2 want;
    const bool possible = lbl_value<ES>(t.value, want); /* can an element of this dtype equal `value` at all? */

    // STEP 1: the segments' aggregates (a segment is uniform over its wavefront: the shuffles are convergent)
    lds[tid] = -1;
    lds[256u + tid] = LDR_NO_KEY;
    __syncthreads();
    for (uint32_t seg = wave; seg < n_seg; seg += LDR_THREADS / 64u) {
        const LdrKeys k = ldr_keys<ES, TO_VALUE>(in, t, seg * 64u + lane, n_el, want, possible);
        int32_t a = k.left, b = k.right;
DEV_UNROLL
        for (uint32_t d = 32u; d >= 1u; d >>= 1) {
            a = ldr_max(a, __shfl_xor(a, (int)d));
            b = ldr_min(b, __shfl_xor(b, (int)d));
        }
        if (lane == 0u) {
            lds[seg] = a;
            lds[256u + seg] = b;
        }
    }
    __syncthreads();

    // STEP 2: lane s scans the aggregates: what comes into segment s from the left (a maximum) and from the right (a minimum)
    {
        int32_t a = lds[tid], b = lds[256u + tid];
DEV_UNROLL
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const int32_t oa = __shfl_up(a, d), ob = __shfl_down(b, d);
            if (lane >= d) a = ldr_max(a, oa);
            if (lane + d < 64u) b = ldr_min(b, ob);
        }
        if (lane == 63u) lds[512u + wave] = a;
        if (lane == 0u) lds[516u + wave] = b;
        int32_t ea = __shfl_up(a, 1u), eb = __shfl_down(b, 1u); /* exclusive */
        if (lane == 0u) ea = -1;
        if (lane == 63u) eb = LDR_NO_KEY;
        __syncthreads();
DEV_UNROLL
        for (uint32_t w = 0; w < LDR_THREADS / 64u; w++) {
            if (w < wave) ea = ldr_max(ea, lds[512u + w]);
            if (w > wave) eb = ldr_min(eb, lds[516u + w]);
        }
        lds[tid] = ea;
        lds[256u + tid] = eb;
    }
    __syncthreads();

    // STEP 3: every segment again: the inclusive scans, the carries, the store
    for (uint32_t seg = wave; seg < n_seg; seg += LDR_THREADS / 64u) {
        const uint32_t i = seg * 64u + lane;
        const LdrKeys k = ldr_keys<ES, TO_VALUE>(in, t, i, n_el, want, possible);
        int32_t a = k.left, b = k.right;
DEV_UNROLL
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const int32_t oa = __shfl_up(a, d), ob = __shfl_down(b, d);
            if (lane >= d) a = ldr_max(a, oa);
            if (lane + d < 64u) b = ldr_min(b, ob);
        }
        a = ldr_max(a, lds[seg]);
        b = ldr_min(b, lds[256u + seg]);
        if (i < n_el) {
            // an odd maximum is a flagged element at or left of i, an even minimum one at or right of it (LDR_NO_KEY is odd);
            // under DIFFERS the site is the element beyond the flagged one
            uint32_t d = LDG_NONE;
            if (a >= 0 && (a & 1)) d = i - ((uint32_t)a >> 1) + (TO_VALUE ? 0u : 1u);
            if (!(b & 1)) {
                const uint32_t dr = ((uint32_t)b >> 1) - i + (TO_VALUE ? 0u : 1u);
                d = dr < d ? dr : d;
            }
            gp[i] = (uint16_t)(d | k.above);
        }
    }
    __syncthreads(); /* the carries are free for the next task */
}

__global__ void __launch_bounds__(LDR_THREADS)
debig_png_label_distance_rows_kernel(const uint8_t *__restrict__ labels, uint8_t *__restrict__ g,
                                     const debig_png_label_distance_rows_task *__restrict__ tasks, uint32_t n_tasks)
{
    __shared__ int32_t lds_scan[520];
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_distance_rows_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!ldr_task_ok(t, labels, g)) continue;
        if (t.sites == 0u) {
            if (t.dtype == 0u) ldr_run<1u, false>(lds_scan, labels, g, t, tid);
            else if (t.dtype == 1u) ldr_run<2u, false>(lds_scan, labels, g, t, tid);
            else if (t.dtype == 2u) ldr_run<4u, false>(lds_scan, labels, g, t, tid);
            else ldr_run<8u, false>(lds_scan, labels, g, t, tid);
        } else {
            if (t.dtype == 0u) ldr_run<1u, true>(lds_scan, labels, g, t, tid);
            else if (t.dtype == 1u) ldr_run<2u, true>(lds_scan, labels, g, t, tid);
            else if (t.dtype == 2u) ldr_run<4u, true>(lds_scan, labels, g, t, tid);
            else ldr_run<8u, true>(lds_scan, labels, g, t, tid);
        }
    }
}

// floor(num / den), den > 0 (C++ division truncates towards zero)
DEV_INLINE int32_t ldc_floor_div(int32_t num, int32_t den)
{
    const int32_t q = num / den;
    return (num % den != 0 && num < 0) ? q - 1 : q;
}

// what the call writes for a squared distance d2 (none: the element has no site), as the 4 bytes of the output element
DEV_INLINE uint32_t ldc_result(bool none, uint32_t d2, uint32_t cap, uint32_t format)
{
    const uint32_t c2 = cap * cap;
    uint32_t r = none ? (cap ? c2 : 0x7fffffffu) : (cap && c2 < d2 ? c2 : d2);
    if (format == 0u) return r;
    if (none && cap == 0u) return 0x7f800000u; /* +infinity */
    const float f = (float)sqrt((double)r);
    uint32_t bits;
    memcpy(&bits, &f, 4);
    return bits;
}

// one column of one task (x: the column in the image)
DEV_INLINE void ldc_column(const uint16_t *__restrict__ gp, uint32_t *op, const debig_png_label_distance_cols_task &t, uint32_t x)
{
    const uint32_t W = t.w, H = t.h;
    const uint16_t *gc = gp + x;
    uint32_t *oc = op + x;
    uint32_t y = 0u;            /* the next row the forward scan fetches */
    uint32_t a = 0u;            /* the run's first row */
    uint32_t n = 0u, vt = 0u;   /* entries of the stack (the top in registers); vt: entry 0 is the virtual site of row a - 1 */
    int32_t ts = 0, tt = 0, tg = 0; /* the top: its site's row, the first row it serves, its row distance */
    int32_t cs = 0, cg = 0;     /* the candidate */
    bool pending = false, closing = false, backward = false;
    uint32_t u = 0u;            /* the row the backward scan writes */
    for (;;) {
        if (!backward) {
            if (!pending) { /* fetch */
                if (y == H) {
                    backward = true;
                    u = H - 1u;
                    continue;
                }
                const uint32_t gv = gc[(uint64_t)y * W];
                if (y > a && (gv & LDG_ABOVE)) { /* the run ends in front of row y, which is its lower virtual site */
                    cs = (int32_t)y;
                    cg = 0;
                    pending = closing = true;
                } else {
                    if ((gv & LDG_NONE) != LDG_NONE) {
                        cs = (int32_t)y;
                        cg = (int32_t)(gv & LDG_NONE);
                        pending = true;
                    }
                    y++;
                }
            }
            if (pending) { /* one pop, or the push */
                bool pop = false;
                if (n == 0u) {
                    ts = cs; tt = (int32_t)a; tg = cg;
                    n = 1u;
                    vt = 0u;
                    pending = false;
                } else if ((tt - ts) * (tt - ts) + tg * tg > (tt - cs) * (tt - cs) + cg * cg) {
                    pop = true;
                } else {
                    const int32_t w = 1 + ldc_floor_div(cs * cs - ts * ts + cg * cg - tg * tg, 2 * (cs - ts));
                    if (w < (int32_t)H) {
                        if (!(n == 1u && vt)) oc[(uint64_t)(a + n - 1u - vt) * W] = (uint32_t)ts | ((uint32_t)tt << 16);
                        ts = cs; tt = w; tg = cg;
                        n++;
                    }
                    pending = false;
                }
                if (pop) {
                    n--;
                    if (n == 1u && vt) {
                        ts = (int32_t)a - 1; tt = (int32_t)a; tg = 0;
                    } else if (n > 0u) {
                        const uint32_t e = oc[(uint64_t)(a + n - 1u - vt) * W];
                        ts = (int32_t)(e & 0xffffu);
                        tt = (int32_t)(e >> 16);
                        tg = (int32_t)(gc[(uint64_t)ts * W] & LDG_NONE);
                    }
                }
                if (!pending && closing) {
                    closing = false;
                    backward = true;
                    u = y - 1u;
                }
            }
        } else {
            bool pop = false, wrote = false;
            if (n == 0u) {
                oc[(uint64_t)u * W] = ldc_result(true, 0u, t.cap, t.format);
                wrote = true;
            } else if (tt > (int32_t)u) { /* an entry that starts behind the run */
                pop = true;
            } else {
                const int32_t du = (int32_t)u - ts;
                oc[(uint64_t)u * W] = ldc_result(false, (uint32_t)(du * du + tg * tg), t.cap, t.format);
                wrote = true;
                pop = tt == (int32_t)u;
            }
            if (pop) {
                n--;
                if (n == 1u && vt) {
                    ts = (int32_t)a - 1; tt = (int32_t)a; tg = 0;
                } else if (n > 0u) {
                    const uint32_t e = oc[(uint64_t)(a + n - 1u - vt) * W];
                    ts = (int32_t)(e & 0xffffu);
                    tt = (int32_t)(e >> 16);
                    tg = (int32_t)(gc[(uint64_t)ts * W] & LDG_NONE);
                }
            }
            if (wrote) {
                if (u == a) {
                    if (y == H) return;
                    backward = false; /* the next run starts in row y, seeded with the virtual site of the row above it */
                    a = y;
                    n = 1u;
                    vt = 1u;
                    ts = (int32_t)a - 1; tt = (int32_t)a; tg = 0;
                } else {
                    u--;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(LDC_THREADS)
debig_png_label_distance_cols_kernel(const uint8_t *__restrict__ g, uint8_t *out, const debig_png_label_distance_cols_task *__restrict__ tasks,
                                     uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_distance_cols_task t = tasks[ti];
        if (!ldc_task_ok(t, g, out)) continue;
        if (tid < t.cols)
            ldc_column(reinterpret_cast<const uint16_t *>(g + t.g_off), reinterpret_cast<uint32_t *>(out + t.out_off), t, t.x0 + tid);
    }
}
