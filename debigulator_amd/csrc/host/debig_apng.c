/*
 * debig_apng_info_get / debig_apng_decode_batch (include/decode_png.h): animated PNG to composited RGBA8 frames.
 * Not a reference function.
 *
 * Host side (plain C): the chunk walk of the still-image decode (spec_walk), then the animation rules over its chunk list.
 * A FRAME is one unit of the pipeline of debig_png_decode_batch: one gather target, one inflate stream, one Adler-32
 * span and de-filter tasks routed as for a still image (tuned kernels or the general one), which write the frame's RGBA8
 * pixels into a frame arena on the device (c->rgba, behind the frame table).  Then one composite launch
 * (debig_hip_apng_composite_batch) renders every file's canvases into c->anim, which goes down in one download.  All
 * frames of all files go through each launch together.
 */
#include <stdlib.h>
#include <string.h>
#include "decode_png.h"
#include "debig_ctx.h"
#include "debig_png_spec.h"

typedef struct apng_frame {
    debig_apng_frame fc;            /* the fcTL fields (a still file: the whole canvas, NONE / SOURCE) */
    uint32_t first_piece, n_pieces; /* the frame's stream: pieces of the file's list, in file order */
    uint64_t z_total, scan;
    uint64_t in_off, out_off, scratch_off, rgba_off; /* device layout */
} apng_frame;

typedef struct apng_file {
    spec_file s; /* the still-image walk: chunks, IDAT payloads, palette, key, routing */
    uint32_t status;
    debig_apng_info ai;
    apng_frame *fr;
    spec_piece *pc;
    uint32_t n_fr, cap_fr, n_pc, cap_pc;
    uint64_t out_bytes, canvas_off, ftab_off;
} apng_file;

static void apng_free(apng_file *A)
{
    spec_free(&A->s);
    free(A->fr);
    free(A->pc);
    A->fr = NULL;
    A->pc = NULL;
}

static int add_frame(apng_file *A, const debig_apng_frame *fc)
{
    if (!spec_grow((void **)&A->fr, &A->cap_fr, A->n_fr, sizeof(apng_frame))) return 0;
    apng_frame *f = &A->fr[A->n_fr++];
    memset(f, 0, sizeof *f);
    f->fc = *fc;
    f->first_piece = A->n_pc;
    return 1;
}

/* a payload piece of the last frame */
static int add_piece(apng_file *A, uint64_t off, uint64_t len)
{
    if (!spec_grow((void **)&A->pc, &A->cap_pc, A->n_pc, sizeof(spec_piece))) return 0;
    A->pc[A->n_pc].off = off;
    A->pc[A->n_pc].len = len;
    A->n_pc++;
    A->fr[A->n_fr - 1].n_pieces++;
    A->fr[A->n_fr - 1].z_total += len;
    return 1;
}

/* the last frame is the IDAT image */
static int take_idat(apng_file *A)
{
    for (uint32_t j = 0; j < A->s.n_idat; j++)
        if (!add_piece(A, A->s.idat[j].off, A->s.idat[j].len)) return 0;
    return 1;
}

/* The animation rules (decode_png.h) over the chunk list of a walk that passed.  DEBIG_PNG_OK or E_ANIM. */
static uint32_t apng_walk(const uint8_t *in, apng_file *A)
{
    const spec_file *F = &A->s;
    const uint32_t W = F->info.width, H = F->info.height;
    int animated = 0;
    for (uint32_t j = 0; j < F->n_chunks; j++) animated |= !memcmp(in + F->chunks[j].off, "acTL", 4);
    if (!animated) {
        debig_apng_frame fc;
        memset(&fc, 0, sizeof fc);
        fc.width = W;
        fc.height = H;
        A->ai.num_frames = 1;
        A->ai.default_is_frame = 1;
        return add_frame(A, &fc) && take_idat(A) ? DEBIG_PNG_OK : DEBIG_PNG_E_CHUNK;
    }
    int seen_idat = 0, n_actl = 0, cur_after = 0; /* cur_after: the last fcTL came after the first IDAT */
    uint32_t seq = 0, n_before = 0, cur_fdat = 0;
    for (uint32_t j = 0; j < F->n_chunks; j++) {
        const uint8_t *type = in + F->chunks[j].off, *body = type + 4;
        const uint64_t len = F->chunks[j].len - 4u;
        if (!memcmp(type, "IDAT", 4)) {
            if (!seen_idat && A->n_fr) { /* an fcTL in front of the IDAT: the IDAT image is frame 0 */
                A->ai.default_is_frame = 1;
                if (!take_idat(A)) return DEBIG_PNG_E_CHUNK;
            }
            seen_idat = 1;
        } else if (!memcmp(type, "acTL", 4)) {
            if (seen_idat || n_actl++ || len != 8) return DEBIG_PNG_E_ANIM;
            A->ai.num_frames = spec_be32(body);
            A->ai.num_plays = spec_be32(body + 4);
            if (!A->ai.num_frames) return DEBIG_PNG_E_ANIM;
        } else if (!memcmp(type, "fcTL", 4)) {
            if (len != 26 || spec_be32(body) != seq++) return DEBIG_PNG_E_ANIM;
            debig_apng_frame fc;
            memset(&fc, 0, sizeof fc);
            fc.width = spec_be32(body + 4);
            fc.height = spec_be32(body + 8);
            fc.x_off = spec_be32(body + 12);
            fc.y_off = spec_be32(body + 16);
            fc.delay_num = (uint16_t)((body[20] << 8) | body[21]);
            fc.delay_den = (uint16_t)((body[22] << 8) | body[23]);
            fc.dispose_op = body[24];
            fc.blend_op = body[25];
            if (!fc.width || !fc.height || (uint64_t)fc.x_off + fc.width > W || (uint64_t)fc.y_off + fc.height > H ||
                fc.dispose_op > 2 || fc.blend_op > 1)
                return DEBIG_PNG_E_ANIM;
            if (!seen_idat) {
                if (n_before++ || fc.x_off || fc.y_off || fc.width != W || fc.height != H) return DEBIG_PNG_E_ANIM;
            } else if (cur_after && !cur_fdat) {
                return DEBIG_PNG_E_ANIM; /* the frame in front of this one has no fdAT */
            }
            if (!add_frame(A, &fc)) return DEBIG_PNG_E_CHUNK;
            cur_after = seen_idat;
            cur_fdat = 0;
        } else if (!memcmp(type, "fdAT", 4)) {
            if (!seen_idat || len < 4 || !cur_after || spec_be32(body) != seq++) return DEBIG_PNG_E_ANIM;
            cur_fdat++;
            if (len > 4 && !add_piece(A, F->chunks[j].off + 8u, len - 4u)) return DEBIG_PNG_E_CHUNK;
        }
    }
    if (cur_after && !cur_fdat) return DEBIG_PNG_E_ANIM;
    if (A->n_fr != A->ai.num_frames) return DEBIG_PNG_E_ANIM;
    return DEBIG_PNG_OK;
}

/* the walk and the animation rules */
static uint32_t apng_parse(const uint8_t *in, uint64_t size, apng_file *A)
{
    uint32_t st = spec_walk(in, size, &A->s, 0);
    A->ai.png = A->s.info;
    if (st == DEBIG_PNG_OK) st = apng_walk(in, A);
    return st;
}

DEBIG_API uint32_t debig_apng_info_get(const uint8_t *p, uint64_t size, debig_apng_info *info, debig_apng_frame *frames,
                                       uint32_t max_frames)
{
    apng_file A;
    memset(&A, 0, sizeof A);
    const uint32_t st = apng_parse(p, size, &A);
    if (info) *info = A.ai;
    if (frames)
        for (uint32_t k = 0; k < A.n_fr && k < max_frames; k++) frames[k] = A.fr[k].fc;
    apng_free(&A);
    return st;
}

/* byte k of frame f's stream (k < z_total) */
static uint8_t frame_z_byte(const apng_file *A, const apng_frame *f, const uint8_t *in, uint64_t k)
{
    for (uint32_t i = 0; i < f->n_pieces; i++) {
        const spec_piece *p = &A->pc[f->first_piece + i];
        if (k < p->len) return in[p->off + k];
        k -= p->len;
    }
    return 0;
}

/* the host rules after the walk: every frame's zlib header (the first failing frame decides), the output size */
static uint32_t apng_host_rules(apng_file *A, const uint8_t *in, const uint8_t *out, uint64_t out_cap)
{
    for (uint32_t k = 0; k < A->n_fr; k++) {
        const apng_frame *f = &A->fr[k];
        if (f->z_total < 2 || !spec_zlib_header_ok(frame_z_byte(A, f, in, 0), frame_z_byte(A, f, in, 1))) return DEBIG_PNG_E_ZLIB;
    }
    const uint64_t wh = (uint64_t)A->s.info.width * A->s.info.height; /* < 2^62 */
    A->out_bytes = wh > UINT64_MAX / 4u / A->n_fr ? UINT64_MAX : wh * 4u * A->n_fr;
    if (!out || out_cap < A->out_bytes) return DEBIG_PNG_E_OUTPUT;
    for (uint32_t k = 0; k < A->n_fr; k++) A->fr[k].scan = spec_scan_bytes(&A->s.info, A->fr[k].fc.width, A->fr[k].fc.height);
    return DEBIG_PNG_OK;
}

DEBIG_API int debig_apng_decode_batch(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                                      const uint64_t *out_caps, uint32_t *status, debig_apng_info *infos, uint32_t n,
                                      uint32_t flags)
{
    if (n == 0) return 0;
    apng_file *A = (apng_file *)calloc(n, sizeof(apng_file));
    uint32_t *live = (uint32_t *)calloc(n, sizeof(uint32_t)); /* files still good, in order */
    apng_frame **gf = NULL;   /* frames of the files still good, file by file */
    uint32_t *gfile = NULL;   /* ... and their files */
    debig_span *spans = NULL;
    uint32_t *sums = NULL, *adl = NULL;
    debig_copy *copies = NULL;
    debig_stream *desc = NULL;
    debig_result *res = NULL;
    debig_png_image *img = NULL;
    debig_png_result *ires = NULL;
    debig_png_spec_task *tasks = NULL;
    debig_png_spec_result *tres = NULL;
    uint32_t *task_file = NULL, *img_file = NULL;
    debig_apng_frame_desc *ftab = NULL;
    debig_apng_task *ctasks = NULL;
    uint8_t **dn_dst = NULL;
    uint64_t *dn_size = NULL, *dn_off = NULL, *up_size = NULL, *up_off = NULL;
    int rc = 2;
    if (!A || !live) goto done;
    rc = 0;
    /* ---- host rules */
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
        apng_file *a = &A[i];
        a->status = apng_parse(inputs[i], input_sizes[i], a);
        if (a->status == DEBIG_PNG_OK) a->status = apng_host_rules(a, inputs[i], outs[i], out_caps[i]);
        if (a->status == DEBIG_PNG_OK) live[m++] = i;
    }
    if (m == 0) goto report; /* nothing for the device */
    debig_ctx *c = debig_ctx_get(0);
    if (!c) { rc = 1; goto done; }
    /* ---- device layout: whole files (c->files); frame streams (c->in); per file in c->out its palette, per frame the
     *      scanline stream (+ 16 readable bytes) and the scratch rings of its general-kernel tasks; in c->rgba the frame
     *      table, then every frame's RGBA8 pixels (16-byte aligned); in c->anim every file's canvases */
    uint32_t nf = 0, n_chunks = 0, n_pieces = 0, n_tasks = 0, n_img = 0;
    for (uint32_t k = 0; k < m; k++) nf += A[live[k]].n_fr;
    const uint64_t ftab_bytes = debig_align16((uint64_t)nf * sizeof(debig_apng_frame_desc));
    uint64_t files_total = 0, in_total = 0, out_total = 64, rgba_total = ftab_bytes, anim_total = 0;
    {
        uint32_t q = 0;
        for (uint32_t k = 0; k < m; k++) {
            apng_file *a = &A[live[k]];
            a->s.general = spec_is_general(&a->s, flags);
            a->s.file_off = files_total;
            files_total += debig_align16(input_sizes[live[k]]) + 16;
            a->s.pal_off = out_total;
            if (a->s.info.color_type == 3) out_total += 1024;
            a->ftab_off = (uint64_t)q * sizeof(debig_apng_frame_desc);
            a->canvas_off = anim_total;
            anim_total += debig_align16(a->out_bytes) + 16;
            n_chunks += a->s.n_chunks;
            n_pieces += a->n_pc;
            for (uint32_t j = 0; j < a->n_fr; j++, q++) {
                apng_frame *f = &a->fr[j];
                f->in_off = in_total;
                in_total += debig_align16(f->z_total) + 32;
                f->out_off = out_total;
                out_total += debig_align16(f->scan) + 32;
                f->scratch_off = out_total;
                if (a->s.general) {
                    uint32_t nt;
                    out_total += spec_general_scratch(&a->s.info, f->fc.width, f->fc.height, &nt);
                    n_tasks += nt;
                } else {
                    n_img++;
                }
                f->rgba_off = rgba_total;
                rgba_total += debig_align16((uint64_t)f->fc.width * f->fc.height * 4u) + 16;
            }
        }
    }
    gf = (apng_frame **)calloc(nf, sizeof(apng_frame *));
    gfile = (uint32_t *)calloc(nf, sizeof(uint32_t));
    spans = (debig_span *)calloc((size_t)n_chunks + nf, sizeof(debig_span));
    sums = (uint32_t *)calloc((size_t)n_chunks + nf, sizeof(uint32_t));
    adl = (uint32_t *)calloc(nf, sizeof(uint32_t));
    copies = (debig_copy *)calloc((size_t)n_pieces + 1, sizeof(debig_copy));
    desc = (debig_stream *)calloc(nf, sizeof(debig_stream));
    res = (debig_result *)calloc(nf, sizeof(debig_result));
    img = (debig_png_image *)calloc((size_t)n_img + 1, sizeof(debig_png_image));
    ires = (debig_png_result *)calloc((size_t)n_img + 1, sizeof(debig_png_result));
    img_file = (uint32_t *)calloc((size_t)n_img + 1, sizeof(uint32_t));
    tasks = (debig_png_spec_task *)calloc((size_t)n_tasks + 1, sizeof(debig_png_spec_task));
    tres = (debig_png_spec_result *)calloc((size_t)n_tasks + 1, sizeof(debig_png_spec_result));
    task_file = (uint32_t *)calloc((size_t)n_tasks + 1, sizeof(uint32_t));
    ftab = (debig_apng_frame_desc *)calloc(nf, sizeof(debig_apng_frame_desc));
    up_size = (uint64_t *)calloc(n, sizeof(uint64_t));
    up_off = (uint64_t *)calloc(n, sizeof(uint64_t));
    dn_dst = (uint8_t **)calloc(n, sizeof(uint8_t *));
    dn_size = (uint64_t *)calloc(n, sizeof(uint64_t));
    dn_off = (uint64_t *)calloc(n, sizeof(uint64_t));
    if (!gf || !gfile || !spans || !sums || !adl || !copies || !desc || !res || !img || !ires || !img_file || !tasks ||
        !tres || !task_file || !ftab || !up_size || !up_off || !dn_dst || !dn_size || !dn_off) {
        rc = 2;
        goto done;
    }
    if ((rc = debig_devbuf_reserve(&c->files, files_total + 64)) || (rc = debig_devbuf_reserve(&c->in, in_total + 64)) ||
        (rc = debig_devbuf_reserve(&c->out, out_total + 64)) || (rc = debig_devbuf_reserve(&c->rgba, rgba_total + 64)) ||
        (rc = debig_devbuf_reserve(&c->anim, anim_total + 64)) ||
        (rc = debig_devbuf_reserve(&c->spans, ((uint64_t)n_chunks + nf) * sizeof(debig_span))) ||
        (rc = debig_devbuf_reserve(&c->crcs, ((uint64_t)n_chunks + nf) * sizeof(uint32_t))) ||
        (rc = debig_devbuf_reserve(&c->copies, ((uint64_t)n_pieces + 1) * sizeof(debig_copy))))
        goto done;
    /* ---- whole files up; chunk CRCs and every frame's stream gathered on the device */
    for (uint32_t k = 0; k < m; k++) {
        up_size[live[k]] = input_sizes[live[k]];
        up_off[live[k]] = A[live[k]].s.file_off;
    }
    if ((rc = debig_upload_packed(c, c->files.ptr, inputs, up_size, up_off, n, files_total))) goto done;
    {
        uint32_t ci = 0, pi = 0;
        for (uint32_t k = 0; k < m; k++) {
            apng_file *a = &A[live[k]];
            for (uint32_t j = 0; j < a->s.n_chunks; j++, ci++) {
                spans[ci].off = a->s.file_off + a->s.chunks[j].off;
                spans[ci].len = a->s.chunks[j].len;
            }
            for (uint32_t j = 0; j < a->n_fr; j++) {
                const apng_frame *f = &a->fr[j];
                uint64_t dst = f->in_off;
                for (uint32_t p = 0; p < f->n_pieces; p++, pi++) {
                    const spec_piece *s = &a->pc[f->first_piece + p];
                    copies[pi].src_off = a->s.file_off + s->off;
                    copies[pi].dst_off = dst;
                    copies[pi].len = s->len;
                    dst += s->len;
                }
            }
        }
        if ((rc = debig_hip_memcpy_h2d(c->spans.ptr, spans, (uint64_t)n_chunks * sizeof(debig_span), NULL)) ||
            (rc = debig_hip_checksum_batch(c->files.ptr, (const debig_span *)c->spans.ptr, (uint32_t *)c->crcs.ptr, n_chunks, 0, NULL)) ||
            (rc = debig_hip_memcpy_d2h(sums, c->crcs.ptr, (uint64_t)n_chunks * sizeof(uint32_t), NULL)) ||
            (n_pieces && (rc = debig_hip_memcpy_h2d(c->copies.ptr, copies, (uint64_t)n_pieces * sizeof(debig_copy), NULL))) ||
            (n_pieces && (rc = debig_hip_gather(c->files.ptr, c->in.ptr, (const debig_copy *)c->copies.ptr, n_pieces, NULL))) ||
            (rc = debig_hip_stream_sync(NULL)))
            goto done;
        ci = 0;
        for (uint32_t k = 0; k < m; k++) {
            apng_file *a = &A[live[k]];
            for (uint32_t j = 0; j < a->s.n_chunks; j++, ci++)
                if (a->status == DEBIG_PNG_OK && sums[ci] != a->s.chunks[j].crc) a->status = DEBIG_PNG_E_CRC;
        }
    }
    /* ---- inflate: every frame of the files still good, plain RFC 1951 into exactly its scanline stream */
    uint32_t ns = 0;
    for (uint32_t k = 0; k < m; k++) {
        apng_file *a = &A[live[k]];
        if (a->status != DEBIG_PNG_OK) continue;
        for (uint32_t j = 0; j < a->n_fr; j++) {
            apng_frame *f = &a->fr[j];
            gf[ns] = f;
            gfile[ns] = live[k];
            desc[ns].in_off = f->in_off + 2u;
            desc[ns].in_len = f->z_total - 2u;
            desc[ns].out_off = f->out_off;
            desc[ns].out_cap = f->scan;
            desc[ns].flags = DEBIG_STREAM_NO_REF_GATES | DEBIG_STREAM_IMAGE_ROWS;
            ns++;
        }
    }
    if (ns == 0) goto report;
    if ((rc = debig_launch_inflate_planned(c, c->in.ptr, desc, res, ns))) goto done;
    for (uint32_t q = 0; q < ns; q++) { /* the inflate step: the first failing frame of a file decides */
        apng_file *a = &A[gfile[q]];
        if (a->status != DEBIG_PNG_OK) continue;
        if (!res[q].good) a->status = res[q].status == DEBIG_E_OUTPUT_FULL ? DEBIG_PNG_E_DATA_LONG : DEBIG_PNG_E_INFLATE;
        else if (res[q].final_size < gf[q]->scan) a->status = DEBIG_PNG_E_DATA_SHORT;
    }
    /* ---- Adler-32: the trailers on the host, the sums of the scanline streams on the device */
    uint32_t na = 0;
    for (uint32_t q = 0; q < ns; q++) {
        apng_file *a = &A[gfile[q]];
        const apng_frame *f = gf[q];
        if (a->status != DEBIG_PNG_OK) continue;
        const uint64_t t = 2u + (res[q].in_end_bits + 7u) / 8u; /* the Adler-32 trailer, in the frame's stream */
        if (t + 4u > f->z_total) { a->status = DEBIG_PNG_E_ADLER; continue; }
        const uint8_t *in = inputs[gfile[q]];
        sums[na] = ((uint32_t)frame_z_byte(a, f, in, t) << 24) | ((uint32_t)frame_z_byte(a, f, in, t + 1) << 16) |
                   ((uint32_t)frame_z_byte(a, f, in, t + 2) << 8) | frame_z_byte(a, f, in, t + 3);
        spans[na].off = f->out_off;
        spans[na].len = f->scan;
        gf[na] = gf[q];
        gfile[na++] = gfile[q];
    }
    if (na &&
        ((rc = debig_hip_memcpy_h2d(c->spans.ptr, spans, (uint64_t)na * sizeof(debig_span), NULL)) ||
         (rc = debig_hip_checksum_batch(c->out.ptr, (const debig_span *)c->spans.ptr, (uint32_t *)c->crcs.ptr, na, 1, NULL)) ||
         (rc = debig_hip_memcpy_d2h(adl, c->crcs.ptr, (uint64_t)na * sizeof(uint32_t), NULL)) ||
         (rc = debig_hip_stream_sync(NULL))))
        goto done;
    for (uint32_t q = 0; q < na; q++)
        if (adl[q] != sums[q] && A[gfile[q]].status == DEBIG_PNG_OK) A[gfile[q]].status = DEBIG_PNG_E_ADLER;
    ns = 0; /* the frames of the files still good */
    for (uint32_t q = 0; q < na; q++) {
        if (A[gfile[q]].status != DEBIG_PNG_OK) continue;
        gf[ns] = gf[q];
        gfile[ns++] = gfile[q];
    }
    if (ns == 0) goto report;
    /* ---- de-filter, routed per file as for a still image, into the frame arena */
    for (uint32_t k = 0; k < m; k++) {
        const apng_file *a = &A[live[k]];
        if (a->status == DEBIG_PNG_OK && a->s.info.color_type == 3 &&
            (rc = debig_hip_memcpy_h2d((uint8_t *)c->out.ptr + a->s.pal_off, a->s.pal, 1024, NULL)))
            goto done;
    }
    n_img = n_tasks = 0;
    for (uint32_t q = 0; q < ns; q++) {
        const apng_file *a = &A[gfile[q]];
        const apng_frame *f = gf[q];
        if (!a->s.general) {
            debig_png_image *im = &img[n_img];
            im->stream_off = f->out_off;
            im->rgba_off = f->rgba_off;
            im->width = f->fc.width;
            im->height = f->fc.height;
            im->color_type = a->s.info.color_type;
            img_file[n_img++] = gfile[q];
            continue;
        }
        const uint32_t nt = spec_image_tasks(&a->s, f->fc.width, f->fc.height, f->out_off, f->rgba_off, f->scratch_off, &tasks[n_tasks]);
        for (uint32_t j = 0; j < nt; j++) task_file[n_tasks + j] = gfile[q];
        n_tasks += nt;
    }
    if (n_img) {
        if ((rc = debig_devbuf_reserve(&c->img, (uint64_t)n_img * sizeof(debig_png_image))) ||
            (rc = debig_devbuf_reserve(&c->imgres, (uint64_t)n_img * sizeof(debig_png_result))) ||
            (rc = debig_hip_memcpy_h2d(c->img.ptr, img, (uint64_t)n_img * sizeof(debig_png_image), NULL)) ||
            (rc = debig_hip_png_defilter_batch(c->out.ptr, c->rgba.ptr, (const debig_png_image *)c->img.ptr,
                                               (debig_png_result *)c->imgres.ptr, n_img, NULL)) ||
            (rc = debig_hip_memcpy_d2h(ires, c->imgres.ptr, (uint64_t)n_img * sizeof(debig_png_result), NULL)))
            goto done;
    }
    if (n_tasks) {
        if ((rc = debig_devbuf_reserve(&c->spec_tasks, (uint64_t)n_tasks * sizeof(debig_png_spec_task))) ||
            (rc = debig_devbuf_reserve(&c->spec_res, (uint64_t)n_tasks * sizeof(debig_png_spec_result))) ||
            (rc = debig_hip_memcpy_h2d(c->spec_tasks.ptr, tasks, (uint64_t)n_tasks * sizeof(debig_png_spec_task), NULL)) ||
            (rc = debig_hip_png_spec_defilter_batch(c->out.ptr, c->rgba.ptr, (const debig_png_spec_task *)c->spec_tasks.ptr,
                                                    (debig_png_spec_result *)c->spec_res.ptr, n_tasks, NULL)) ||
            (rc = debig_hip_memcpy_d2h(tres, c->spec_res.ptr, (uint64_t)n_tasks * sizeof(debig_png_spec_result), NULL)))
            goto done;
    }
    if ((rc = debig_hip_stream_sync(NULL))) goto done;
    for (uint32_t k = 0; k < n_img; k++)
        if (!ires[k].good) A[img_file[k]].status = DEBIG_PNG_E_FILTER;
    for (uint32_t j = 0; j < n_tasks; j++) { /* a filter error in any frame outranks a palette error in any frame */
        apng_file *a = &A[task_file[j]];
        if (tres[j].status == DEBIG_PNG_SPEC_E_FILTER) a->status = DEBIG_PNG_E_FILTER;
        else if (tres[j].status == DEBIG_PNG_SPEC_E_PALETTE && a->status == DEBIG_PNG_OK) a->status = DEBIG_PNG_E_PALETTE;
    }
    /* ---- compositing: the frame table in front of the frame arena, one task per DEBIG_APNG_TASK_PX canvas pixels */
    {
        uint64_t n_ct = 0;
        for (uint32_t k = 0; k < m; k++) {
            const apng_file *a = &A[live[k]];
            if (a->status == DEBIG_PNG_OK)
                n_ct += ((uint64_t)a->s.info.width * a->s.info.height + DEBIG_APNG_TASK_PX - 1u) / DEBIG_APNG_TASK_PX;
        }
        if (n_ct > 0xffffffffu) { rc = 2; goto done; }
        if (n_ct) {
            ctasks = (debig_apng_task *)calloc((size_t)n_ct, sizeof(debig_apng_task));
            if (!ctasks) { rc = 2; goto done; }
            uint32_t ct = 0;
            for (uint32_t k = 0; k < m; k++) {
                const apng_file *a = &A[live[k]];
                if (a->status != DEBIG_PNG_OK) continue;
                debig_apng_frame_desc *d = ftab + a->ftab_off / sizeof(debig_apng_frame_desc);
                for (uint32_t j = 0; j < a->n_fr; j++) {
                    const apng_frame *f = &a->fr[j];
                    d[j].rgba_off = f->rgba_off;
                    d[j].x_off = f->fc.x_off;
                    d[j].y_off = f->fc.y_off;
                    d[j].width = f->fc.width;
                    d[j].height = f->fc.height;
                    d[j].dispose_op = f->fc.dispose_op;
                    d[j].blend_op = f->fc.blend_op;
                }
                const uint64_t wh = (uint64_t)a->s.info.width * a->s.info.height;
                for (uint64_t p0 = 0; p0 < wh; p0 += DEBIG_APNG_TASK_PX) {
                    debig_apng_task *t = &ctasks[ct++];
                    t->out_off = a->canvas_off;
                    t->ftab_off = a->ftab_off;
                    t->px0 = p0;
                    t->n_px = (uint32_t)(wh - p0 < DEBIG_APNG_TASK_PX ? wh - p0 : DEBIG_APNG_TASK_PX);
                    t->n_frames = a->n_fr;
                    t->width = a->s.info.width;
                    t->height = a->s.info.height;
                }
            }
            if ((rc = debig_devbuf_reserve(&c->anim_tasks, (uint64_t)ct * sizeof(debig_apng_task))) ||
                (rc = debig_hip_memcpy_h2d(c->rgba.ptr, ftab, (uint64_t)nf * sizeof(debig_apng_frame_desc), NULL)) ||
                (rc = debig_hip_memcpy_h2d(c->anim_tasks.ptr, ctasks, (uint64_t)ct * sizeof(debig_apng_task), NULL)) ||
                (rc = debig_hip_apng_composite_batch(c->rgba.ptr, c->anim.ptr, (const debig_apng_task *)c->anim_tasks.ptr, ct, NULL)))
                goto done;
        }
    }
    /* ---- canvases down */
    {
        uint64_t last_end = 0;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = live[k];
            if (A[i].status != DEBIG_PNG_OK) continue;
            dn_dst[i] = outs[i];
            dn_size[i] = A[i].out_bytes;
            dn_off[i] = A[i].canvas_off;
            if (dn_off[i] + dn_size[i] > last_end) last_end = dn_off[i] + dn_size[i];
        }
        if (last_end && (rc = debig_download_unpack(c, c->anim.ptr, dn_dst, dn_size, dn_off, n, last_end))) goto done;
    }
report:
    for (uint32_t i = 0; i < n; i++) {
        status[i] = A[i].status;
        if (infos) infos[i] = A[i].ai;
    }
done:
    if (A)
        for (uint32_t i = 0; i < n; i++) apng_free(&A[i]);
    free(A);
    free(live);
    free(gf);
    free(gfile);
    free(spans);
    free(sums);
    free(adl);
    free(copies);
    free(desc);
    free(res);
    free(img);
    free(ires);
    free(img_file);
    free(tasks);
    free(tres);
    free(task_file);
    free(ftab);
    free(ctasks);
    free(up_size);
    free(up_off);
    free(dn_dst);
    free(dn_size);
    free(dn_off);
    return rc;
}
