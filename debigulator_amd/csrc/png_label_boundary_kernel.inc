// png_label_boundary_kernel.inc -- boundary bands of a dense label tensor: void / ignore rings (RING) and edge maps (EDGE)
// (include/decode_png.h: debig_png_label_boundary, which has the rule; include/debig_hip.h: debig_hip_png_label_boundary_batch and
// the task).
//
// Element (x, y) is a boundary element iff an element at (x + dx, y + dy), |dy| <= radius, |dx| <= reach[|dy|], inside the image,
// differs from it.  One TASK is a tile of one image for one workgroup of 256 lanes, in two passes over LDS:
//   - STAGE: the tile plus a halo of `radius` elements on every side, clipped at the image, goes into the VALUE plane at the
//     element's own width, one element per lane and step (coalesced loads, conflict-free stores).  Every staged row starts at the
//     same byte shift (below 16), chosen so that the 16-byte items of the plane are the 16-byte items of the output row y0;
//   - PASS 1: for every element of the tile's columns in every staged row, the distance along the row to the nearest element in
//     the image that differs from it, capped at radius + 1, one byte per element in the DIST plane (the value plane's geometry
//     divided by the element size).  A lane takes one element; its 2 x radius reads run along the row, conflict-free;
//   - PASS 2: a lane takes one 16-byte ITEM of a tile row (16 / 8 / 4 / 2 elements) and, for each of the 2 x radius + 1 rows of
//     the window that lie in the image, reads the item of that row (one 16-byte read at a 16-byte aligned address: sixteen lanes
//     cover a bank row) and its dist bytes (one read of 16 / 8 / 4 / 2 bytes).  Element j is boundary iff, in some row, the element
//     above or below it differs from it, or equals it and has a row distance <= reach[|dy|];
//   - STORE: RING writes boundary ? value : the element, EDGE one byte 1 / 0.  An item whose elements all lie in the tile and
//     whose output address is aligned goes out as one store (16 bytes under RING, 16 / 8 / 4 / 2 under EDGE), every other item
//     element by element.  Which store an item takes depends on addresses only; the bytes are the same.
// The reach table travels in registers (seventeen bytes as two 64-bit words and one more); the kernel knows nothing about shapes.
// A task that breaks a bound is skipped (never indexed out of range).  Nothing waits on another workgroup.  No scratch, no inline
// assembly, plain vector loads and stores.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs inflate_kernel.inc and png_stage_common.inc in
// front of it.

#define LBD_THREADS 256u
#define LBD_LDS_ITEMS (DEBIG_PNG_LABEL_BOUNDARY_LDS_BYTES / 16u)

// where a task's staged window lies and how the two planes are laid out (all uniform over the workgroup)
struct LbdGeo {
    uint32_t sx0, sy0, sw, sh; /* the staged window: columns sx0 .. sx0 + sw - 1, rows sy0 .. sy0 + sh - 1 of the image */
    uint32_t pitch, dpitch;    /* bytes of a row of the value plane and of the dist plane, multiples of 16 */
    uint32_t dist0;            /* byte offset of the dist plane in LDS */
};

DEV_INLINE LbdGeo lbd_geo(const debig_png_label_boundary_task &t)
{
    LbdGeo g;
    const uint32_t r = t.radius, es = 1u << t.dtype;
    g.sx0 = t.x0 > r ? t.x0 - r : 0u;
    g.sy0 = t.y0 > r ? t.y0 - r : 0u;
    const uint32_t sx1 = t.x0 + t.tile_w + r < t.w ? t.x0 + t.tile_w + r : t.w;
    const uint32_t sy1 = t.y0 + t.tile_h + r < t.h ? t.y0 + t.tile_h + r : t.h;
    g.sw = sx1 - g.sx0;
    g.sh = sy1 - g.sy0;
    g.pitch = (g.sw * es + 30u) & ~15u; /* a shift of at most 15 bytes in front, whole items behind */
    g.dpitch = (g.pitch / es + 15u) & ~15u;
    g.dist0 = g.sh * g.pitch;
    return g;
}

DEV_INLINE bool lbd_task_ok(const debig_png_label_boundary_task &t, const uint8_t *labels, const uint8_t *out)
{
    if (t.dtype > 3u || t.mode > 1u || t.radius == 0u || t.radius > DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS) return false;
    for (uint32_t d = 0; d <= DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS; d++)
        if (d <= t.radius && t.reach[d] > t.radius) return false;
    if (!stage_dim_ok(t.w, t.h)) return false;
    if (t.tile_w == 0u || t.tile_w > DEBIG_PNG_LABEL_BOUNDARY_MAX_TILE || t.tile_h == 0u || t.tile_h > DEBIG_PNG_LABEL_BOUNDARY_MAX_TILE)
        return false;
    if (t.x0 >= t.w || t.tile_w > t.w - t.x0 || t.y0 >= t.h || t.tile_h > t.h - t.y0) return false;
    const LbdGeo g = lbd_geo(t);
    if (g.dist0 + g.sh * g.dpitch > DEBIG_PNG_LABEL_BOUNDARY_LDS_BYTES) return false;
    if (t.mode == 0u) { /* RING: the value is an element of the dtype */
        if (t.dtype == 0u && (t.value < 0 || t.value > 255)) return false;
        if (t.dtype == 1u && (t.value < 0 || t.value > 65535)) return false;
        if (t.dtype == 2u && (t.value < -2147483647 - 1 || t.value > 2147483647)) return false;
    }
    const uint64_t es1 = (1u << t.dtype) - 1u, os1 = t.mode == 0u ? es1 : 0u;
    return stage_addr_ok(labels, t.label_off, es1) && stage_addr_ok(out, t.out_off, os1);
}

// the reach table in registers: entry 0 in the low byte of lo; next() drops the entry in front
struct LbdReach {
    uint64_t lo, hi;
    uint32_t top;
    DEV_MEMBER_INLINE LbdReach(const debig_png_label_boundary_task &t) : lo(0u), hi(0u), top(t.reach[16])
    {
DEV_UNROLL
        for (uint32_t d = 0; d < 8u; d++) {
            lo |= (uint64_t)t.reach[d] << (8u * d);
            hi |= (uint64_t)t.reach[8u + d] << (8u * d);
        }
    }
    __device__ __forceinline__ uint32_t front() const { return (uint32_t)lo & 255u; }
    __device__ __forceinline__ void next()
    {
        lo = (lo >> 8) | (hi << 56);
        hi = (hi >> 8) | ((uint64_t)top << 56);
        top = 0u;
    }
};

// N bytes (16, 8, 4 or 2) at p, aligned to N, into the low bytes of w[4] / out of them
template <uint32_t N>
DEV_INLINE void lbd_load_bytes(const uint8_t *p, uint32_t (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (N == 16u) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else if (N == 8u) {
        const uint2 q = *reinterpret_cast<const uint2 *>(p);
        w[0] = q.x; w[1] = q.y;
    } else if (N == 4u) {
        w[0] = *reinterpret_cast<const uint32_t *>(p);
    } else {
        w[0] = *reinterpret_cast<const uint16_t *>(p);
    }
}

template <uint32_t N>
DEV_INLINE void lbd_store_bytes(uint8_t *p, const uint32_t (&w)[4])
{
    if (N == 16u) {
        uint4 q;
        q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
        *reinterpret_cast<uint4 *>(p) = q;
    } else if (N == 8u) {
        uint2 q;
        q.x = w[0]; q.y = w[1];
        *reinterpret_cast<uint2 *>(p) = q;
    } else if (N == 4u) {
        *reinterpret_cast<uint32_t *>(p) = w[0];
    } else {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)w[0];
    }
}

// one row of the window into the boundary bits of an item: bit j is set when element j of the row's item q differs from element
// j of the centre item c, or equals it and has a row distance (dd, one byte per element) <= reach
template <uint32_t ES>
DEV_INLINE uint32_t lbd_row_bits(const uint8_t *lds, const LbdGeo &g, uint32_t row, uint32_t ib, const uint32_t (&c)[4], uint32_t reach)
{
    constexpr uint32_t EPI = 16u / ES;
    uint32_t q[4], dd[4], bits = 0u;
    lbd_load_bytes<16u>(lds + row * g.pitch + ib, q);
    lbd_load_bytes<EPI>(lds + g.dist0 + row * g.dpitch + ib / ES, dd);
DEV_UNROLL
    for (uint32_t j = 0; j < EPI; j++) {
        const uint2 a = lbl_item_get<ES>(q, j), b = lbl_item_get<ES>(c, j);
        const uint32_t d = (dd[j >> 2] >> (8u * (j & 3u))) & 255u;
        bits |= (uint32_t)(!lbl_same(a, b) || d <= reach) << j;
    }
    return bits;
}

// one task; ES: bytes of an element, EDGE: the output is one byte 1 / 0 per element (else the element or `value`)
template <uint32_t ES, bool EDGE>
DEV_INLINE void lbd_run(uint8_t *lds, const uint8_t *__restrict__ labels, uint8_t *__restrict__ out, const debig_png_label_boundary_task &t,
                        uint32_t tid)
{
    constexpr uint32_t EPI = 16u / ES, OS = EDGE ? 1u : ES;
    const LbdGeo g = lbd_geo(t);
    const uint32_t r = t.radius, W = t.w;
    const uint8_t *in = labels + t.label_off;
    uint8_t *o = out + t.out_off;
    // the byte shift of every staged row: element (sx0, y0) of the OUTPUT starts an item of the plane where it starts one in memory
    const uint64_t e00 = (uint64_t)t.y0 * W + g.sx0;
    const uint32_t shift = EDGE ? (uint32_t)(((uintptr_t)o + e00) & (EPI - 1u)) * ES : (uint32_t)(((uintptr_t)o + e00 * ES) & 15u);

    // STAGE
    {
        StageWalk at(tid, g.sw, LBD_THREADS);
        for (uint32_t i = tid; i < g.sw * g.sh; i += LBD_THREADS) {
            const uint2 v = lbl_load<ES>(in + ((uint64_t)(g.sy0 + at.r) * W + g.sx0 + at.x) * ES);
            lbl_store<ES>(lds + at.r * g.pitch + shift + at.x * ES, v);
            at.next();
        }
    }
    __syncthreads();

    // PASS 1: row distances of the tile's columns in every staged row
    {
        const uint32_t c0 = t.x0 - g.sx0; /* the tile's first column in the window */
        StageWalk at(tid, t.tile_w, LBD_THREADS);
        for (uint32_t i = tid; i < t.tile_w * g.sh; i += LBD_THREADS) {
            const uint32_t c = c0 + at.x; /* the window holds columns c - r .. c + r as far as the image has them */
            const uint8_t *row = lds + at.r * g.pitch + shift;
            const uint2 v = lbl_load<ES>(row + c * ES);
            uint32_t d = r + 1u;
            for (uint32_t k = r; k >= 1u; k--) { /* from far to near: the nearest one is written last */
                bool differs = false;
                if (c >= k) {
                    const uint2 u = lbl_load<ES>(row + (c - k) * ES);
                    differs = !lbl_same(u, v);
                }
                if (c + k < g.sw) {
                    const uint2 u = lbl_load<ES>(row + (c + k) * ES);
                    differs = differs || !lbl_same(u, v);
                }
                if (differs) d = k;
            }
            lds[g.dist0 + at.r * g.dpitch + shift / ES + c] = (uint8_t)d;
            at.next();
        }
    }
    __syncthreads();

    // PASS 2 and STORE: the items of the tile's rows
    {
        const uint32_t b0 = shift + (t.x0 - g.sx0) * ES, b1 = b0 + t.tile_w * ES; /* the tile's bytes in a row of the plane */
        const uint32_t i0 = b0 >> 4, ni = ((b1 + 15u) >> 4) - i0;
        const uint32_t cy0 = t.y0 - g.sy0; /* the tile's first row in the window */
        uint2 val;
        val.x = (uint32_t)(uint64_t)t.value;
        val.y = (uint32_t)((uint64_t)t.value >> 32);
        StageWalk at(tid, ni, LBD_THREADS);
        for (uint32_t i = tid; i < ni * t.tile_h; i += LBD_THREADS) {
            const uint32_t ib = (i0 + at.x) << 4, cy = cy0 + at.r;
            uint32_t c[4];
            lbd_load_bytes<16u>(lds + cy * g.pitch + ib, c);
            LbdReach reach(t);
            uint32_t bits = lbd_row_bits<ES>(lds, g, cy, ib, c, reach.front());
            for (uint32_t d = 1u; d <= r; d++) {
                reach.next();
                if (cy >= d) bits |= lbd_row_bits<ES>(lds, g, cy - d, ib, c, reach.front());
                if (cy + d < g.sh) bits |= lbd_row_bits<ES>(lds, g, cy + d, ib, c, reach.front());
            }
            // the item's elements: column x_first + j of the image, those inside the tile count
            const int32_t x_first = (int32_t)g.sx0 + ((int32_t)ib - (int32_t)shift) / (int32_t)ES;
            uint32_t inside = 0u;
DEV_UNROLL
            for (uint32_t j = 0; j < EPI; j++) {
                const int32_t x = x_first + (int32_t)j;
                inside |= (uint32_t)(x >= (int32_t)t.x0 && x < (int32_t)(t.x0 + t.tile_w)) << j;
            }
            uint32_t res[4] = {0u, 0u, 0u, 0u};
DEV_UNROLL
            for (uint32_t j = 0; j < EPI; j++) {
                if (EDGE) res[j >> 2] |= ((bits >> j) & 1u) << (8u * (j & 3u));
                else lbl_item_put<ES>(res, j, (bits >> j) & 1u ? val : lbl_item_get<ES>(c, j));
            }
            uint8_t *dst = o + ((int64_t)((uint64_t)(t.y0 + at.r) * W) + x_first) * (int64_t)OS;
            constexpr uint32_t NB = EPI * OS; /* bytes of an item's results */
            if (inside == (EPI == 16u ? 0xffffu : (1u << EPI) - 1u) && ((uintptr_t)dst & (NB - 1u)) == 0u) {
                lbd_store_bytes<NB>(dst, res);
            } else {
DEV_UNROLL
                for (uint32_t j = 0; j < EPI; j++)
                    if ((inside >> j) & 1u) lbl_store<OS>(dst + (int64_t)j * OS, lbl_item_get<OS>(res, j));
            }
            at.next();
        }
    }
    __syncthreads(); /* the planes are free for the next task */
}

__global__ void __launch_bounds__(LBD_THREADS)
debig_png_label_boundary_kernel(const uint8_t *__restrict__ labels, uint8_t *__restrict__ out,
                                const debig_png_label_boundary_task *__restrict__ tasks, uint32_t n_tasks)
{
    __shared__ uint4 lds_planes[LBD_LDS_ITEMS]; /* the value plane, the dist plane behind it */
    uint8_t *lds = reinterpret_cast<uint8_t *>(lds_planes);
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_boundary_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (!lbd_task_ok(t, labels, out)) continue;
        if (t.mode == 0u) {
            if (t.dtype == 0u) lbd_run<1u, false>(lds, labels, out, t, tid);
            else if (t.dtype == 1u) lbd_run<2u, false>(lds, labels, out, t, tid);
            else if (t.dtype == 2u) lbd_run<4u, false>(lds, labels, out, t, tid);
            else lbd_run<8u, false>(lds, labels, out, t, tid);
        } else {
            if (t.dtype == 0u) lbd_run<1u, true>(lds, labels, out, t, tid);
            else if (t.dtype == 1u) lbd_run<2u, true>(lds, labels, out, t, tid);
            else if (t.dtype == 2u) lbd_run<4u, true>(lds, labels, out, t, tid);
            else lbd_run<8u, true>(lds, labels, out, t, tid);
        }
    }
}
