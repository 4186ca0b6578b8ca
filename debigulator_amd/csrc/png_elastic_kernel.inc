// png_elastic_kernel.inc -- the four warp kernels under an ELASTIC deformation (torchvision ElasticTransform, MONAI Rand2DElastic):
// crop + affine warp displaced by a smooth per-file field, of decoded PNG pixels into one dense tensor, with or without the
// colour matrix, and of raw and colour-coded labels into one dense integer tensor (include/decode_png.h:
// debig_png_decode_batch_tensor_elastic, debig_png_decode_batch_labels_elastic, debig_png_decode_batch_color_labels_elastic;
// include/debig_hip.h: debig_hip_png_elastic_batch, debig_hip_png_elastic_color_batch, debig_hip_png_label_elastic_batch,
// debig_hip_png_color_label_elastic_batch).
//
// The arithmetic is fixed by decode_png.h: a grid of grid_h x grid_w nodes spans the output from edge to edge, each node a
// displacement (dx, dy) in output pixels as Q16 int32 (at most 2^28 in magnitude).  Per output pixel and axis: the cell k and
// the Q14 fraction t by two 32-bit divisions, four Catmull-Rom weights from t in integers (their sum is exactly 16384), then
// D = (sum_i sum_j wy_i wx_j d[i][j] + 2^27) >> 28 over the 4 x 4 nodes around the cell, edge nodes replicated, in int64 with
// nothing rounded in between.  (U, V) = the affine (NU, NV) of m[] plus the linear part of m[] applied to (Dx, Dy).  Everything
// around (U, V) is the affine warp's, word for word: the kernel bodies of png_warp_kernel.inc, png_color_kernel.inc and
// png_color_label_warp_kernel.inc are instantiated with the map policy of this file (WarpElastic).
//   - a TASK is the warp task of the kernel it mirrors, field for field, followed by field_off (bytes from the launch's `fields`
//     argument, 8-byte aligned; UINT64_MAX: no field, which is a field of zeros) and grid_w, grid_h; tasks, workgroups and the
//     lane mapping are the warp kernels' (one lane per output pixel, lanes along X and on into the next row, 256 lanes);
//   - the workgroup STAGES its task's grid in LDS (at most 33 x 33 x 8 = 8712 bytes) and keeps it while consecutive tasks name
//     the same field_off and grid size (ela_hold_grid, the scheme of clbl_hold_map); the staging pass compares every node with
//     the limit and the workgroup votes through one LDS word, so a task with a node out of range is skipped by every lane;
//   - the map policy has STATE here (the LDS pointers, the fields, what is held); the bodies take it by value, and the affine and
//     projective policies are empty types whose hold step is `true`;
//   - per pixel: four 32-bit divisions, two weight quadruples (a few 64-bit multiplies), 16 eight-byte LDS reads at addresses
//     that neighbouring lanes share or that lie in neighbouring nodes (a wavefront covers at most a few cells of a row: the
//     reads are broadcasts), 32 multiply-adds of int32 x int32 into int64 and 8 of int64 x int32.
// A task that breaks a bound -- those of its warp counterpart, a grid dimension outside 2 .. 33, a misaligned field_off, a
// staged node above 2^28 in magnitude -- is skipped (never indexed out of range).  No scratch, no inline assembly, plain vector
// stores only, no atomics beyond the warp twin's `unmatched` add.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_warp_kernel.inc, png_color_kernel.inc and
// png_color_label_warp_kernel.inc in front of it.

#define ELA_GRID_MIN 2u
#define ELA_GRID_MAX 33u
#define ELA_NODE_MAX ((int32_t)1 << 28)
#define ELA_NO_FIELD (~(uint64_t)0)

// one node: (dx, dy) in Q16, read and staged as one 8-byte word
struct __attribute__((aligned(8))) ElaNode { int32_t x, y; };

// the cell k (at most g - 2) and the Q14 fraction t (0 .. 16384) of output coordinate X on an axis of W pixels and g nodes:
// (2X + 1)(g - 1) < 2^21 and rem 2^14 + W < 2^30, so 32 bits hold everything
DEV_INLINE void ela_cell(uint32_t X, uint32_t W, uint32_t g, uint32_t &k, uint32_t &t)
{
    const uint32_t num = (2u * X + 1u) * (g - 1u), den = 2u * W;
    k = num / den;
    t = ((num - k * den) * 16384u + W) / den;
}

// the four Q14 weights of the Keys kernel (a = -1/2) at fraction t, for the nodes k - 1 .. k + 2: three rounded, the anchor (w1,
// node k's, when t < 8192, else w2) takes what is missing to 16384
struct ElaW { int32_t w0, w1, w2, w3; };
DEV_INLINE ElaW ela_weights(uint32_t t)
{
    const int64_t T = (int64_t)t, t2 = T * T, t3 = t2 * T, half = (int64_t)1 << 28;
    ElaW q;
    q.w0 = (int32_t)((-t3 + 2 * t2 * 16384 - T * ((int64_t)1 << 28) + half) >> 29);
    q.w1 = (int32_t)((3 * t3 - 5 * t2 * 16384 + ((int64_t)1 << 43) + half) >> 29);
    q.w2 = (int32_t)((-3 * t3 + 4 * t2 * 16384 + T * ((int64_t)1 << 28) + half) >> 29);
    q.w3 = (int32_t)((t3 - t2 * 16384 + half) >> 29);
    if (t < 8192u) q.w1 = 16384 - (q.w0 + q.w2 + q.w3);
    else q.w2 = 16384 - (q.w0 + q.w1 + q.w3);
    return q;
}

// node k - 1 + j of an axis of g nodes, clamped into the grid (the edge nodes are replicated)
DEV_INLINE uint32_t ela_node(uint32_t k, uint32_t j, uint32_t g)
{
    const uint32_t a = k + j; // the node plus one
    return a == 0u ? 0u : a > g ? g - 1u : a - 1u;
}

// the displacement (Dx, Dy) of output pixel (X, Y) in Q16, from the staged grid (row major, (dx, dy) per node)
template <class Task>
DEV_INLINE void ela_displacement(const ElaNode *grid, const Task &t, uint32_t X, uint32_t Y, int64_t &Dx, int64_t &Dy)
{
    const uint32_t gw = t.grid_w, gh = t.grid_h;
    uint32_t kx, tx, ky, ty;
    ela_cell(X, t.out_w, gw, kx, tx);
    ela_cell(Y, t.out_h, gh, ky, ty);
    const ElaW wx = ela_weights(tx), wy = ela_weights(ty);
    const uint32_t c0 = ela_node(kx, 0u, gw), c1 = ela_node(kx, 1u, gw), c2 = ela_node(kx, 2u, gw), c3 = ela_node(kx, 3u, gw);
    const int32_t wyv[4] = {wy.w0, wy.w1, wy.w2, wy.w3};
    int64_t sx = 0, sy = 0;
    RSZ_UNROLL
    for (uint32_t i = 0; i < 4u; i++) {
        const ElaNode *row = grid + ela_node(ky, i, gh) * gw;
        const ElaNode d0 = row[c0], d1 = row[c1], d2 = row[c2], d3 = row[c3];
        const int64_t rx = (int64_t)wx.w0 * d0.x + (int64_t)wx.w1 * d1.x + (int64_t)wx.w2 * d2.x + (int64_t)wx.w3 * d3.x;
        const int64_t ry = (int64_t)wx.w0 * d0.y + (int64_t)wx.w1 * d1.y + (int64_t)wx.w2 * d2.y + (int64_t)wx.w3 * d3.y;
        sx += rx * wyv[i];
        sy += ry * wyv[i];
    }
    Dx = (sx + ((int64_t)1 << 27)) >> 28;
    Dy = (sy + ((int64_t)1 << 27)) >> 28;
}

// what a task adds to the bounds of its warp twin, as far as the task alone tells (uniform over the workgroup)
template <class Task>
DEV_INLINE bool ela_task_ok(const Task &t)
{
    return t.grid_w >= ELA_GRID_MIN && t.grid_w <= ELA_GRID_MAX && t.grid_h >= ELA_GRID_MIN && t.grid_h <= ELA_GRID_MAX &&
           (t.field_off == ELA_NO_FIELD || !(t.field_off & 7u));
}

// the grid a workgroup holds in LDS: staged when the task's field offset or grid size differs from the one held -> whether
// every node of it lies within the limit (the workgroup's vote; a held grid keeps its verdict).  The caller has checked
// ela_task_ok; every lane must be here (the task loop is uniform)
struct ElaHeld {
    uint64_t off;
    uint32_t gw, gh; /* gw == 0: none yet */
    bool ok;
};
template <class Task>
DEV_INLINE bool ela_hold_grid(ElaNode *lds_grid, uint32_t *lds_bad, ElaHeld &held, const Task &t, const uint8_t *__restrict__ fields,
                              uint32_t tid)
{
    if (t.field_off == held.off && t.grid_w == held.gw && t.grid_h == held.gh) return held.ok;
    __syncthreads(); /* nobody still reads the grid that goes, or the vote of its staging */
    if (tid == 0u) *lds_bad = 0u;
    __syncthreads();
    const uint32_t nodes = (uint32_t)t.grid_w * t.grid_h;
    bool bad = false;
    if (t.field_off == ELA_NO_FIELD) {
        for (uint32_t k = tid; k < nodes; k += WARP_THREADS) lds_grid[k] = ElaNode{0, 0};
    } else {
        const ElaNode *gf = reinterpret_cast<const ElaNode *>(fields + t.field_off);
        for (uint32_t k = tid; k < nodes; k += WARP_THREADS) {
            const ElaNode d = gf[k];
            bad = bad || d.x < -ELA_NODE_MAX || d.x > ELA_NODE_MAX || d.y < -ELA_NODE_MAX || d.y > ELA_NODE_MAX;
            lds_grid[k] = d;
        }
    }
    if (bad) *lds_bad = 1u; /* (every writer stores the same word) */
    __syncthreads();
    held.off = t.field_off;
    held.gw = t.grid_w;
    held.gh = t.grid_h;
    held.ok = *lds_bad == 0u;
    return held.ok;
}

// the elastic map as the policy the kernel bodies take (png_warp_kernel.inc has the scheme): ela_task_ok among the skips, the
// task's grid held in LDS that the kernel owns, (U, V) displaced -- behind hold(), which returned true.  The one policy with state
struct WarpElastic {
    ElaNode *grid;
    uint32_t *bad;
    const uint8_t *fields;
    ElaHeld held;
    DEV_MEMBER_INLINE WarpElastic(ElaNode *lds_grid, uint32_t *lds_bad, const uint8_t *fields_)
        : grid(lds_grid), bad(lds_bad), fields(fields_), held{0u, 0u, 0u, false} {}
    template <class Task>
    static DEV_MEMBER_INLINE bool task_ok(const Task &t) { return ela_task_ok(t); }
    template <class Task> // (forced inline in the emulator build as well, which would otherwise export it)
    __device__ __forceinline__ bool hold(const Task &t, uint32_t tid) { return ela_hold_grid(grid, bad, held, t, fields, tid); }
    template <class Task>
    DEV_MEMBER_INLINE void uv(const Task &t, uint32_t X, uint32_t Y, int64_t cx, int64_t cy, int64_t &U, int64_t &V) const
    {
        int64_t Dx, Dy;
        ela_displacement(grid, t, X, Y, Dx, Dy);
        U = warp_nu(t, cx, cy) + ((t.m[0] * Dx + t.m[1] * Dy + 16384) >> 15);
        V = warp_nv(t, cx, cy) + ((t.m[3] * Dx + t.m[4] * Dy + 16384) >> 15);
    }
};

// ---- the four kernels: the body of each kind under the elastic map, the grid and the vote in LDS of their own --------------------

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_elastic_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, const debig_png_elastic_task *__restrict__ tasks,
                         const uint8_t *__restrict__ fields, uint32_t n_tasks)
{
    __shared__ ElaNode lds_grid[ELA_GRID_MAX * ELA_GRID_MAX];
    __shared__ uint32_t lds_bad;
    warp_image_tasks(WarpElastic(lds_grid, &lds_bad, fields), src, out, tasks, n_tasks);
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_elastic_color_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                               const debig_png_elastic_color_task *__restrict__ tasks, const uint8_t *__restrict__ weights,
                               const uint8_t *__restrict__ fields, uint32_t n_tasks)
{
    __shared__ ElaNode lds_grid[ELA_GRID_MAX * ELA_GRID_MAX];
    __shared__ uint32_t lds_bad;
    warp_color_tasks(WarpElastic(lds_grid, &lds_bad, fields), src, out, tasks, weights, n_tasks);
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_label_elastic_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                               const debig_png_label_elastic_task *__restrict__ tasks, const int32_t *__restrict__ lut,
                               const uint8_t *__restrict__ fields, uint32_t n_tasks)
{
    __shared__ int32_t lds_lut[256];
    __shared__ ElaNode lds_grid[ELA_GRID_MAX * ELA_GRID_MAX];
    __shared__ uint32_t lds_bad;
    warp_label_tasks(WarpElastic(lds_grid, &lds_bad, fields), lds_lut, src, out, tasks, lut, n_tasks);
}

__global__ void __launch_bounds__(WARP_THREADS)
debig_png_color_label_elastic_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                                     const debig_png_color_label_elastic_task *__restrict__ tasks, const uint8_t *__restrict__ tables,
                                     uint32_t *__restrict__ unmatched, const uint8_t *__restrict__ fields, uint32_t n_tasks)
{
    __shared__ uint2 lds_map[DEBIG_PNG_CMAP_MAX_SLOTS]; /* (key, value) per slot */
    __shared__ ElaNode lds_grid[ELA_GRID_MAX * ELA_GRID_MAX];
    __shared__ uint32_t lds_bad;
    clbl_warp_tasks(WarpElastic(lds_grid, &lds_bad, fields), lds_map, src, out, tasks, tables, unmatched, n_tasks);
}
