// png_label_kernel.inc -- crop + nearest pick + class remap + widening of raw PNG labels into one dense integer tensor
// (include/decode_png.h: debig_png_decode_batch_labels; include/debig_hip.h: debig_hip_png_label_gather_batch).
//
// The source is what debig_png_spec_defilter_index_kernel left in the arena: one byte (depths up to 8) or one little-endian
// uint16 (depth 16) per pixel.  Output element (X, Y) of an image is src[sy[Y] * pitch + sx[X]], through the 256-entry LUT
// when the call has one, widened to uint8 / uint16 / int32 / int64.  sx and sy are made on the host (the rule's product needs
// 64 bits; no division runs here), one uint32 table per axis and crop length.
//
// One TASK is a run of output rows of one image; one workgroup of 256 lanes per task:
//   - an ITEM is E adjacent elements of one output row -- E = 8, 8, 4, 2 for uint8, uint16, int32, int64: 8 bytes for uint8,
//     16 bytes for the others -- and the lanes run along x, then on into the next row of the run, so narrow tensors keep every
//     lane busy and a wavefront's stores are adjacent;
//   - a lane loads its E entries of sx as one or two 16-byte (int64: 8-byte) loads, then E source labels of 1 or 2 bytes.
//     sx is monotone: when the call shrinks, the labels a wavefront reads per load instruction walk forward over a few cache
//     lines (64 lanes x E x scale bytes in all); when it enlarges, neighbouring lanes read the same bytes again;
//   - the E results are packed into dwords and stored by spec_store_run (png_spec_kernel.inc), which picks the widest store
//     the address allows: rows of a width that is no multiple of 16 bytes start unaligned, so the width is found per item;
//   - the last item of a row (out_w no multiple of E) goes out element by element;
//   - the LUT (1 KB) is staged in LDS once per workgroup, before the task loop.  Label maps are blocky, so the lanes of a
//     ds_read_b32 mostly hit one address (a broadcast); distinct labels conflict only when they are 32 entries apart.
// A task that breaks a bound is skipped (never indexed out of range).  No atomics, no scratch (every per-item array is indexed
// by unrolled constants), nothing shared between workgroups.
// Included by debig_hip.hip (hipcc) and by the CPU emulator build (tests); needs png_spec_kernel.inc and png_stage_common.inc
// in front of it.

#define LBL_THREADS 256u

// the rows of one task of either gather (this file, png_color_label_kernel.inc): elements of ES bytes, E per item;
// pick(el) -> the element of the source pixel `el` of the crop.  A lane's picks come in the order of its elements.
template <uint32_t ES, uint32_t E, class Task, class Pick>
DEV_INLINE void lbl_gather_rows(const Task &t, uint8_t *__restrict__ out, const uint32_t *__restrict__ sx,
                                const uint32_t *__restrict__ sy, uint32_t tid, Pick pick)
{
    constexpr uint32_t ND = E * ES / 4u; /* dwords of a full item */
    const uint32_t ipr = (t.out_w + E - 1u) / E, n = t.rows * ipr; /* items per row (<= 8192), items of the task */
    StageWalk wk(tid, ipr, LBL_THREADS);
    for (uint32_t i = tid; i < n; i += LBL_THREADS) {
        const uint32_t Y = t.row0 + wk.r, x = wk.x * E;
        const uint64_t srow = (uint64_t)sy[Y] * t.src_pitch;
        uint8_t *o = out + t.out_off + ((uint64_t)Y * t.out_w + x) * ES;
        if (x + E <= t.out_w) {
            uint32_t ix[E], B[ND];
            if (E == 2u) {
                const uint2 q = *reinterpret_cast<const uint2 *>(sx + x);
                ix[0] = q.x; ix[1] = q.y;
            } else {
DEV_UNROLL
                for (uint32_t j = 0; j < E / 4u; j++) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(sx + x + 4u * j);
                    ix[4u * j] = q.x; ix[4u * j + 1u] = q.y; ix[4u * j + 2u] = q.z; ix[4u * j + 3u] = q.w;
                }
            }
DEV_UNROLL
            for (uint32_t j = 0; j < ND; j++) B[j] = 0u;
DEV_UNROLL
            for (uint32_t j = 0; j < E; j++) {
                const uint32_t v = pick(srow + ix[j]);
                if (ES == 1u) B[j / 4u] |= (v & 0xffu) << (8u * (j & 3u));
                else if (ES == 2u) B[j / 2u] |= (v & 0xffffu) << (16u * (j & 1u));
                else if (ES == 4u) B[j] = v;
                else { B[2u * j] = v; B[2u * j + 1u] = (uint32_t)((int32_t)v >> 31); }
            }
            spec_store_run<E * ES>(o, B);
        } else {
DEV_UNROLL
            for (uint32_t j = 0; j < E; j++) {
                if (x + j >= t.out_w) break;
                lbl_store1<ES>(o + j * ES, pick(srow + sx[x + j]));
            }
        }
        wk.next();
    }
}

// the raw-label pick: a source label of SB bytes, through the LUT when there is one
template <uint32_t ES, uint32_t E, uint32_t SB>
DEV_INLINE void lbl_rows(const int32_t *lut, const debig_png_label_task &t, const uint8_t *__restrict__ src,
                         uint8_t *__restrict__ out, const uint32_t *__restrict__ sx, const uint32_t *__restrict__ sy, uint32_t tid)
{
    const uint8_t *s0 = src + t.src_off;
    lbl_gather_rows<ES, E>(t, out, sx, sy, tid, [&](uint64_t el) -> uint32_t {
        const uint32_t v = SB == 1u ? (uint32_t)s0[el] : (uint32_t)reinterpret_cast<const uint16_t *>(s0)[el];
        return lut ? (uint32_t)lut[v & 255u] : v;
    });
}

__global__ void __launch_bounds__(LBL_THREADS)
debig_png_label_gather_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out,
                              const debig_png_label_task *__restrict__ tasks, const uint8_t *__restrict__ tables,
                              const int32_t *__restrict__ lut, uint32_t n_tasks)
{
    __shared__ int32_t lds_lut[256];
    const uint32_t tid = threadIdx.x;
    if (lut) lds_lut[tid & 255u] = lut[tid & 255u];
    __syncthreads();
    const int32_t *L = lut ? lds_lut : nullptr;
    for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
        const debig_png_label_task t = tasks[ti];
        // (uniform over the workgroup: every lane skips, or none)
        if (t.out_w == 0u || t.out_w > 16384u || t.out_h > 16384u || t.rows == 0u || t.row0 >= t.out_h || t.rows > t.out_h - t.row0 ||
            (t.src_bytes != 1u && t.src_bytes != 2u) || t.dtype > 3u || (t.dtype == 0u && t.src_bytes == 2u) ||
            (lut && t.src_bytes == 2u) || ((t.sx_off | t.sy_off) & 15u) || (t.src_off & (t.src_bytes - 1u)))
            continue;
        const uint32_t *sx = reinterpret_cast<const uint32_t *>(tables + t.sx_off);
        const uint32_t *sy = reinterpret_cast<const uint32_t *>(tables + t.sy_off);
        if (t.src_bytes == 1u) {
            if (t.dtype == 0u) lbl_rows<1u, 8u, 1u>(L, t, src, out, sx, sy, tid);
            else if (t.dtype == 1u) lbl_rows<2u, 8u, 1u>(L, t, src, out, sx, sy, tid);
            else if (t.dtype == 2u) lbl_rows<4u, 4u, 1u>(L, t, src, out, sx, sy, tid);
            else lbl_rows<8u, 2u, 1u>(L, t, src, out, sx, sy, tid);
        } else {
            if (t.dtype == 1u) lbl_rows<2u, 8u, 2u>(L, t, src, out, sx, sy, tid);
            else if (t.dtype == 2u) lbl_rows<4u, 4u, 2u>(L, t, src, out, sx, sy, tid);
            else lbl_rows<8u, 2u, 2u>(L, t, src, out, sx, sy, tid);
        }
    }
}
