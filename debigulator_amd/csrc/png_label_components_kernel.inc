// png_label_components_kernel.inc -- connected components of a dense label tensor (include/decode_png.h:
// debig_png_label_components, which has the rule; include/debig_hip.h: debig_hip_png_label_components_*_batch and the task).
// Union-find over a PARENT PLANE, one uint32 per element of the image: the index y * w + x of another element of the same component
// that is not larger than the element's own, or LCC_BG for a background element.  A ROOT is a slot that holds its own index.  Five
// kernels share one TASK, a run of whole rows of one image, at most 16384 elements (or one row), for one workgroup of 256 lanes:
//
// ROWS    parent[p] = the start of p's horizontal run of equal values: an inclusive maximum scan of the key "i where a run starts,
//         else none" over the task's flat range, cut into segments of 64 as in the distance rows pass (per-segment maxima by
//         shuffles, a scan of the at most 256 aggregates, the segments again with their carry).  Every run is a tree of depth 1.
// MERGE   for every element of a row y > 0 the unions with row y - 1 that can add something: the vertical pair in the first column
//         of an overlap of two runs, a diagonal pair (8) only where the element's vertical pair differs and the element beside it
//         does not already carry the link.  lcc_union is the lock-free form (Playne-Komura, ECL-CC): find both roots, atomicMin the
//         smaller into the larger root's slot, and go on from the returned value when the slot was a root no longer.  DURING THIS
//         LAUNCH THE PLANE IS WRITTEN BY AGENT-SCOPE atomicMin ONLY, so every value a slot ever holds is <= every earlier one, <= the
//         slot's index, and an element of the slot's component: a stale read (another XCD's L2; the loads are agent-scope and pass
//         the L1) is still an ancestor, every find strictly descends and ends, and when the launch is over the roots are the
//         components' smallest elements, their FIRSTs.  Path halving in the find of this launch is the same atomicMin.
// COUNT   counts[task] = the roots in the task's rows.  From here on the plane is only read.
// NUMBER  (CONSECUTIVE) base = the sum of the counts of the image's earlier tasks, summed by the task itself (at most 16383 words, 64
//         per lane); a root gets out = base + its rank among the task's roots in raster order + 1 (ballots, one scan of the aggregates).
// FINISH  FIRST: out[p] = find(p), background -1.  CONSECUTIVE: a non-root gets out[find(p)], background 0, roots stay.
//
// EVERY INDEX READ FROM THE PLANE IS CHECKED before it is an address: a value that is not below w * h, or above the slot it came
// from, makes the slot a root (lcc_link), so a wrong plane ends every loop and never leaves the image.  No loop waits for another
// workgroup: an atomicMin that found the slot changed goes on from the smaller index it returned, which is somebody's progress.
// The work is NOT linear for every input: a find walks a tree whose depth depends on the data and on the race.
// A task that breaks a bound is skipped (never indexed out of range).  No scratch, no inline assembly.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc and
// png_stage_common.inc in front of it.

#define LCC_THREADS 256u
#define LCC_BG 0xffffffffu

DEV_INLINE bool lcc_task_ok(const debig_png_label_components_task &t, const void *labels, const void *parent, const void *out, const void *counts)
{
    if (t.dtype > 3u || (t.connectivity != 4u && t.connectivity != 8u) || t.use_background > 1u || t.ids > 1u) return false;
    if (!stage_dim_ok(t.w, t.h) || !stage_rows_ok(t.h, t.row0, t.rows)) return false;
    if (!stage_budget_ok(t.rows, t.w, DEBIG_PNG_LABEL_COMPONENTS_ELEMS)) return false;
    if (t.count_first > t.count_idx || t.count_idx - t.count_first > 16383u) return false;
    // (a kernel hands in NULL for a buffer it does not have: its offset is tested all the same)
    return stage_addr_ok(labels, t.label_off, (1u << t.dtype) - 1u) && stage_addr_ok(parent, t.parent_off, 3u) &&
           stage_addr_ok(out, t.out_off, 3u) && stage_addr_ok(counts, 0u, 3u);
}

// the slot's value as a link: an index below the slot's own and inside the image, or the slot itself (a root, a background
// slot, and whatever a wrong plane holds)
DEV_INLINE uint32_t lcc_link(uint32_t q, uint32_t p, uint32_t n_px) { return (q < p && q < n_px) ? q : p; }

// an agent-scope load of a slot: it passes this CU's L1, which no other CU's atomic refreshes
DEV_INLINE uint32_t lcc_load(const uint32_t *parent, uint32_t p)
{
    return __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above p while the plane changes, halving the path on the way: p's slot gets its grandparent, again by atomicMin
DEV_INLINE uint32_t lcc_find_merge(uint32_t *parent, uint32_t p, uint32_t n_px)
{
    uint32_t q = lcc_link(lcc_load(parent, p), p, n_px);
    while (q != p) {
        const uint32_t g = lcc_link(lcc_load(parent, q), q, n_px);
        if (g == q) break;
        atomicMin(parent + p, g);
        p = q;
        q = g;
    }
    return q;
}

// the root above p in a plane that nobody writes
DEV_INLINE uint32_t lcc_find(const uint32_t *__restrict__ parent, uint32_t p, uint32_t n_px)
{
    for (;;) {
        const uint32_t q = lcc_link(parent[p], p, n_px);
        if (q == p) return p;
        p = q;
    }
}

// a, b < n_px: two elements of one component.  Every trip either ends or goes on with a strictly smaller a.
DEV_INLINE void lcc_union(uint32_t *parent, uint32_t a, uint32_t b, uint32_t n_px)
{
    for (;;) {
        a = lcc_find_merge(parent, a, n_px);
        b = lcc_find_merge(parent, b, n_px);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = atomicMin(parent + a, b); /* b < a */
        if (old >= a) return;                          /* it was a root (or a wrong slot, which counts as one): linked */
        a = old;                                       /* somebody linked it first: their root and b are still to be joined */
    }
}

// what the background is for elements of ES bytes: the value as an element, and whether an element is tested against it at all
struct LccBg { uint2 want; bool on; };

template <uint32_t ES>
DEV_INLINE LccBg lcc_background(const debig_png_label_components_task &t)
{
    LccBg b;
    const bool possible = lbl_value<ES>(t.background, b.want);
    b.on = t.use_background != 0u && possible;
    return b;
}

// ---- ROWS ------------------------------------------------------------------------------------------------------------------------

// the scan key of element i of the flat range: i where a run starts, else -1
template <uint32_t ES>
DEV_INLINE int32_t lcc_key(const uint8_t *in, uint32_t W, uint32_t i, uint32_t n_el)
{
    if (i >= n_el) return -1;
    if (i % W == 0u) return (int32_t)i;
    return lbl_same(lbl_load<ES>(in + (uint64_t)i * ES), lbl_load<ES>(in + (uint64_t)(i - 1u) * ES)) ? -1 : (int32_t)i;
}

// one task; lds: [0, 256) the segments' maxima, then what comes in from the left; [256, 260) the four wavefronts' totals
template <uint32_t ES>
DEV_INLINE void lcc_rows_run(int32_t *lds, const uint8_t *__restrict__ labels, uint8_t *__restrict__ parent,
                             const debig_png_label_components_task &t, uint32_t tid)
{
    const uint32_t W = t.w, n_el = t.rows * W, n_seg = (n_el + 63u) >> 6, p0 = t.row0 * W; /* n_el <= 16384: at most 256 segments */
    const uint8_t *in = labels + t.label_off + (uint64_t)p0 * ES;
    uint32_t *pp = reinterpret_cast<uint32_t *>(parent + t.parent_off) + p0;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const LccBg bg = lcc_background<ES>(t);

    // STEP 1: the segments' maxima (a segment is uniform over its wavefront: the shuffles are convergent)
    lds[tid] = -1;
    __syncthreads();
    for (uint32_t seg = wave; seg < n_seg; seg += LCC_THREADS / 64u) {
        int32_t a = lcc_key<ES>(in, W, seg * 64u + lane, n_el);
DEV_UNROLL
        for (uint32_t d = 32u; d >= 1u; d >>= 1) {
            const int32_t o = __shfl_xor(a, (int)d);
            a = a > o ? a : o;
        }
        if (lane == 0u) lds[seg] = a;
    }
    __syncthreads();

    // STEP 2: lane s scans the aggregates: what comes into segment s from the left
    {
        int32_t a = lds[tid];
DEV_UNROLL
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const int32_t o = __shfl_up(a, d);
            if (lane >= d) a = a > o ? a : o;
        }
        if (lane == 63u) lds[256u + wave] = a;
        int32_t ea = __shfl_up(a, 1u); /* exclusive */
        if (lane == 0u) ea = -1;
        __syncthreads();
DEV_UNROLL
        for (uint32_t w = 0; w < LCC_THREADS / 64u; w++) {
            const int32_t o = lds[256u + w];
            if (w < wave) ea = ea > o ? ea : o;
        }
        lds[tid] = ea;
    }
    __syncthreads();

    // STEP 3: every segment again: the inclusive scan, the carry, the store.  Element 0 starts a run, so no maximum is "none".
    for (uint32_t seg = wave; seg < n_seg; seg += LCC_THREADS / 64u) {
        const uint32_t i = seg * 64u + lane;
        int32_t a = lcc_key<ES>(in, W, i, n_el);
DEV_UNROLL
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const int32_t o = __shfl_up(a, d);
            if (lane >= d) a = a > o ? a : o;
        }
        const int32_t c = lds[seg];
        a = a > c ? a : c;
        if (i < n_el) {
            const bool back = bg.on && lbl_same(lbl_load<ES>(in + (uint64_t)i * ES), bg.want);
            pp[i] = back ? LCC_BG : p0 + (uint32_t)a;
        }
    }
    __syncthreads(); /* the carries are free for the next task */
}

__global__ void __launch_bounds__(LCC_THREADS)
debig_png_label_components_rows_kernel(const uint8_t *__restrict__ labels, uint8_t *__restrict__ parent,
                                       const debig_png_label_components_task *__restrict__ tasks, uint32_t n_tasks)
{
    __shared__ int32_t lds_scan[260];
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_components_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!lcc_task_ok(t, labels, parent, NULL, NULL)) continue;
        if (t.dtype == 0u) lcc_rows_run<1u>(lds_scan, labels, parent, t, tid);
        else if (t.dtype == 1u) lcc_rows_run<2u>(lds_scan, labels, parent, t, tid);
        else if (t.dtype == 2u) lcc_rows_run<4u>(lds_scan, labels, parent, t, tid);
        else lcc_rows_run<8u>(lds_scan, labels, parent, t, tid);
    }
}

// ---- MERGE -----------------------------------------------------------------------------------------------------------------------

template <uint32_t ES>
DEV_INLINE void lcc_merge_run(const uint8_t *__restrict__ labels, uint8_t *parent, const debig_png_label_components_task &t, uint32_t tid)
{
    const uint32_t W = t.w, n_px = W * t.h, p0 = t.row0 * W, p1 = p0 + t.rows * W;
    const uint8_t *in = labels + t.label_off;
    uint32_t *pp = reinterpret_cast<uint32_t *>(parent + t.parent_off);
    const LccBg bg = lcc_background<ES>(t);
    // row 0 of the image has no row above it (the row above a task's first row belongs to the image, if not to the task)
    for (uint32_t p = (p0 ? p0 : W) + tid; p < p1; p += LCC_THREADS) {
        const uint32_t x = p % W;
        const uint2 v = lbl_load<ES>(in + (uint64_t)p * ES);
        if (bg.on && lbl_same(v, bg.want)) continue;
        const bool lft = x > 0u, rgt = x + 1u < W;
        const bool up = lbl_same(v, lbl_load<ES>(in + (uint64_t)(p - W) * ES));
        const bool l = lft && lbl_same(v, lbl_load<ES>(in + (uint64_t)(p - 1u) * ES));
        const bool ul = lft && lbl_same(v, lbl_load<ES>(in + (uint64_t)(p - W - 1u) * ES));
        if (up) {
            // the first column of the overlap of the two runs: the pair to the left is not the same overlap
            if (!(l && ul)) lcc_union(pp, p, p - W, n_px);
        } else if (t.connectivity == 8u) {
            // a diagonal adds something only where the vertical pair differs, and the element beside p, if it is of p's run, has
            // the same link as its own vertical pair
            if (ul && !l) lcc_union(pp, p, p - W - 1u, n_px);
            if (rgt && lbl_same(v, lbl_load<ES>(in + (uint64_t)(p - W + 1u) * ES)) && !lbl_same(v, lbl_load<ES>(in + (uint64_t)(p + 1u) * ES)))
                lcc_union(pp, p, p - W + 1u, n_px);
        }
    }
}

__global__ void __launch_bounds__(LCC_THREADS)
debig_png_label_components_merge_kernel(const uint8_t *__restrict__ labels, uint8_t *parent,
                                        const debig_png_label_components_task *__restrict__ tasks, uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_components_task t = tasks[ti];
        if (!lcc_task_ok(t, labels, parent, NULL, NULL)) continue;
        if (t.dtype == 0u) lcc_merge_run<1u>(labels, parent, t, tid);
        else if (t.dtype == 1u) lcc_merge_run<2u>(labels, parent, t, tid);
        else if (t.dtype == 2u) lcc_merge_run<4u>(labels, parent, t, tid);
        else lcc_merge_run<8u>(labels, parent, t, tid);
    }
}

// ---- COUNT, NUMBER ---------------------------------------------------------------------------------------------------------------

// the sum of one value per lane over the workgroup, in every lane; lds: four words that are free again when it returns
DEV_INLINE uint32_t lcc_sum(uint32_t *lds, uint32_t v, uint32_t tid)
{
DEV_UNROLL
    for (uint32_t d = 32u; d >= 1u; d >>= 1) v += __shfl_xor(v, (int)d);
    if ((tid & 63u) == 0u) lds[tid >> 6] = v;
    __syncthreads();
    const uint32_t s = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(LCC_THREADS)
debig_png_label_components_count_kernel(const uint8_t *__restrict__ parent, uint32_t *__restrict__ counts,
                                        const debig_png_label_components_task *__restrict__ tasks, uint32_t n_tasks)
{
    __shared__ uint32_t lds_sum[4];
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_components_task t = tasks[ti];
        if (!lcc_task_ok(t, NULL, parent, NULL, counts)) continue;
        const uint32_t p0 = t.row0 * t.w, p1 = p0 + t.rows * t.w;
        const uint32_t *pp = reinterpret_cast<const uint32_t *>(parent + t.parent_off);
        uint32_t c = 0u;
        for (uint32_t p = p0 + tid; p < p1; p += LCC_THREADS) c += pp[p] == p;
        c = lcc_sum(lds_sum, c, tid);
        if (tid == 0u) counts[t.count_idx] = c;
    }
}

__global__ void __launch_bounds__(LCC_THREADS)
debig_png_label_components_number_kernel(const uint8_t *__restrict__ parent, const uint32_t *__restrict__ counts, uint8_t *__restrict__ out,
                                         const debig_png_label_components_task *__restrict__ tasks, uint32_t n_tasks)
{
    __shared__ uint32_t lds_rank[260]; /* [0, 256) the segments' roots, then the roots in front of each; [256, 260) sums */
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_components_task t = tasks[ti];
        if (!lcc_task_ok(t, NULL, parent, out, counts)) continue;
        const uint32_t p0 = t.row0 * t.w, n_el = t.rows * t.w, n_seg = (n_el + 63u) >> 6;
        const uint32_t *pp = reinterpret_cast<const uint32_t *>(parent + t.parent_off) + p0;
        int32_t *op = reinterpret_cast<int32_t *>(out + t.out_off) + p0;
        // the image's earlier tasks: at most 16383 counts
        uint32_t base = 0u;
        for (uint32_t k = t.count_first + tid; k < t.count_idx; k += LCC_THREADS) base += counts[k];
        base = lcc_sum(lds_rank + 256, base, tid);
        lds_rank[tid] = 0u;
        __syncthreads();
        for (uint32_t seg = wave; seg < n_seg; seg += LCC_THREADS / 64u) {
            const uint32_t i = seg * 64u + lane;
            const unsigned long long roots = __ballot(i < n_el && pp[i] == p0 + i);
            if (lane == 0u) lds_rank[seg] = (uint32_t)__popcll(roots);
        }
        __syncthreads();
        {   // lane s: the roots of the segments in front of segment s
            const uint32_t own = lds_rank[tid];
            uint32_t a = own;
DEV_UNROLL
            for (uint32_t d = 1u; d < 64u; d <<= 1) {
                const uint32_t o = __shfl_up(a, d);
                if (lane >= d) a += o;
            }
            if (lane == 63u) lds_rank[256u + wave] = a;
            __syncthreads();
DEV_UNROLL
            for (uint32_t w = 0; w < LCC_THREADS / 64u; w++)
                if (w < wave) a += lds_rank[256u + w];
            lds_rank[tid] = a - own;
        }
        __syncthreads();
        for (uint32_t seg = wave; seg < n_seg; seg += LCC_THREADS / 64u) {
            const uint32_t i = seg * 64u + lane;
            const bool root = i < n_el && pp[i] == p0 + i;
            const unsigned long long roots = __ballot(root);
            if (root) op[i] = (int32_t)(base + lds_rank[seg] + (uint32_t)__popcll(roots & ((1ull << lane) - 1ull)) + 1u);
        }
        __syncthreads(); /* the ranks are free for the next task */
    }
}

// ---- FINISH ----------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(LCC_THREADS)
debig_png_label_components_finish_kernel(const uint8_t *__restrict__ parent, uint8_t *out,
                                         const debig_png_label_components_task *__restrict__ tasks, uint32_t n_tasks)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_components_task t = tasks[ti];
        if (!lcc_task_ok(t, NULL, parent, out, NULL)) continue;
        const uint32_t n_px = t.w * t.h, p0 = t.row0 * t.w, p1 = p0 + t.rows * t.w;
        const uint32_t *pp = reinterpret_cast<const uint32_t *>(parent + t.parent_off);
        int32_t *op = reinterpret_cast<int32_t *>(out + t.out_off);
        for (uint32_t p = p0 + tid; p < p1; p += LCC_THREADS) {
            if (pp[p] == LCC_BG) {
                op[p] = t.ids ? 0 : -1;
                continue;
            }
            const uint32_t r = lcc_find(pp, p, n_px);
            if (t.ids == 0u) op[p] = (int32_t)r;
            else if (r != p) op[p] = op[r]; /* a root's number is in place (NUMBER), and no task of this launch writes a root */
        }
    }
}
