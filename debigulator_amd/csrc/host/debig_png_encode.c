/* debig_png_encode_batch, debig_png_encode_batch_dyn and debig_png_encode_batch_lz (include/decode_png.h, which has the rules): dense
 * tensors in device memory -> PNG files in host memory.  The three calls are their argument checks in front of ONE body; levels 2 and 3
 * differ from it in the DEFLATE launch -- debig_hip_png_encode_dynamic_batch (csrc/png_encode_dynamic_kernel.inc) or
 * debig_hip_png_encode_lz_batch (csrc/png_encode_lz_kernel.inc) in rounds of DEBIG_PNG_ENCODE_ROUND_TASKS tasks that share one arena of
 * worst-case token rows --, level 3 in the task's row_stride, and both in the zlib header's second byte.
 * The host checks the descriptors, uploads the two task lists, launches the filter and the deflate kernel
 * (csrc/png_encode_kernel.inc), reads the chunks' byte counts and the range flags back, lays every good file out in a device arena
 * -- what stands in front of and behind the DEFLATE bytes comes from the host, the chunk outputs are moved by debig_hip_gather --,
 * takes the Adler-32 of every filtered stream and the CRC-32 of every IDAT from debig_hip_checksum_batch, and downloads each file
 * once.  It never loops over pixel or stream bytes. */
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "decode_png.h"
#include "debig_ctx.h"

_Static_assert(sizeof(debig_png_encode_filter_task) == 64 && sizeof(debig_png_encode_deflate_task) == 64, "two and four 64-bit fields, the rest uint32");
_Static_assert(sizeof(debig_png_encode_desc) == 48, "eight uint32, two uint64");
_Static_assert(sizeof(debig_png_encode_dynamic_task) == 80 && offsetof(debig_png_encode_dynamic_task, token_off) == 64 &&
                   offsetof(debig_png_encode_dynamic_task, slot_off) == offsetof(debig_png_encode_deflate_task, slot_off) &&
                   offsetof(debig_png_encode_dynamic_task, flags) == offsetof(debig_png_encode_deflate_task, flags),
               "a dynamic task is a deflate task and its token row");
_Static_assert(sizeof(debig_png_encode_lz_task) == 80 && offsetof(debig_png_encode_lz_task, token_off) == 64 &&
                   offsetof(debig_png_encode_lz_task, row_stride) == offsetof(debig_png_encode_dynamic_task, reserved2) &&
                   offsetof(debig_png_encode_lz_task, flags) == offsetof(debig_png_encode_dynamic_task, flags),
               "an lz task is a dynamic task with row_stride in its last word");
#define TOKEN_ROW (4u * (uint64_t)DEBIG_PNG_ENCODE_CHUNK) /* worst case: every byte of a chunk a literal */

static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

static void be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

/* the CRC-32 of the few header bytes the host writes (IHDR, PLTE, tRNS, IEND) */
static uint32_t crc_small(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
    }
    return c ^ 0xffffffffu;
}

/* one chunk at p -> the bytes written */
static size_t put_chunk(uint8_t *p, const char *type, const uint8_t *data, uint32_t len)
{
    be32(p, len);
    memcpy(p + 4, type, 4);
    if (len) memcpy(p + 8, data, len);
    be32(p + 8 + len, crc_small(p + 4, 4u + len));
    return 12u + (size_t)len;
}

static int desc_ok(const debig_png_encode_desc *d)
{
    if (d->width == 0 || d->width > 16384u || d->height == 0 || d->height > 16384u) return 0;
    if (d->channels == 0 || d->channels > 4u || d->dtype > DEBIG_PNG_L_I64 || d->layout > DEBIG_PNG_LAYOUT_CHW) return 0;
    if (d->depth != 8u && d->depth != 16u) return 0;
    if ((d->dtype == DEBIG_PNG_L_U8 && d->depth != 8u) || (d->dtype == DEBIG_PNG_L_U16 && d->depth != 16u)) return 0;
    if (d->dtype >= DEBIG_PNG_L_I32 && d->channels != 1u) return 0;
    if (d->palette_entries > 256u || (d->palette_entries && (d->channels != 1u || d->depth != 8u))) return 0;
    return d->trns_entries <= d->palette_entries;
}

static uint64_t stream_bytes(const debig_png_encode_desc *d) { return (uint64_t)d->height * (1u + (uint64_t)d->width * d->channels * (d->depth / 8u)); }
static uint64_t n_chunks(uint64_t len) { return (len + DEBIG_PNG_ENCODE_CHUNK - 1u) / DEBIG_PNG_ENCODE_CHUNK; }
/* what stands in front of the IDAT chunk */
static uint64_t head_bytes(const debig_png_encode_desc *d)
{
    return 8u + 25u + (d->palette_entries ? 12u + 3u * (uint64_t)d->palette_entries : 0u) + (d->trns_entries ? 12u + (uint64_t)d->trns_entries : 0u);
}

DEBIG_API uint64_t debig_png_encode_bound(const debig_png_encode_desc *d)
{
    if (!d || !desc_ok(d)) return 0;
    const uint64_t len = stream_bytes(d), nc = n_chunks(len);
    /* level 0: five bytes in front of every chunk, the empty stored block behind every chunk but the last; level 1 is never longer */
    return head_bytes(d) + 12u + 2u + len + 5u * nc + 5u * (nc - 1u) + 4u + 12u;
}

typedef struct enc_image {
    uint32_t idx;                     /* the image's place in the call                                       */
    uint64_t stream_off, stream_len;  /* its filtered stream in the arena                                    */
    uint64_t first_task, tasks;       /* its deflate tasks                                                   */
    uint64_t deflate_bytes;           /* what they wrote                                                     */
    uint64_t file_off, file_size;     /* its file in the arena                                               */
    uint64_t head_off;                /* what the host writes, among the uploaded bytes                      */
} enc_image;

/* the slot of deflate task k in the task list (tasks of ts bytes each) */
static uint64_t task_slot_off(const uint8_t *tasks, size_t ts, uint64_t k)
{
    uint64_t v;
    memcpy(&v, tasks + k * ts + offsetof(debig_png_encode_deflate_task, slot_off), sizeof v);
    return v;
}

/* what both calls check before any device work */
static int args_ok(const void *const *d_images, const debig_png_encode_desc *descs, const uint8_t *side, void *const *outs, const uint64_t *out_caps,
                   uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter, uint32_t level, uint32_t top_level)
{
    if (!d_images || !descs || !outs || !out_caps || !out_sizes || !status || filter > DEBIG_PNG_FILTER_ADAPTIVE || level > top_level) return 0;
    for (uint32_t i = 0; i < n; i++)
        if (descs[i].palette_entries && !side) return 0;
    return 1;
}

/* the body of the three calls; level 0 .. 3 */
static int encode_body(const void *const *d_images, const debig_png_encode_desc *descs, const uint8_t *side, void *const *outs,
                       const uint64_t *out_caps, uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter, uint32_t level)
{
    const size_t ts = level >= 2u ? sizeof(debig_png_encode_dynamic_task) : sizeof(debig_png_encode_deflate_task);
    int rc = 2;
    enc_image *im = (enc_image *)calloc(n, sizeof *im);
    uint8_t *blob = NULL, *heads = NULL;
    uint32_t *words = NULL;
    debig_copy *copies = NULL;
    debig_span *spans = NULL;
    if (!im) return rc;
    /* ---- 1. the descriptors; where every good image's stream and slots lie ---- */
    uint32_t n_good = 0;
    uint64_t n_ft = 0, n_dt = 0, at = 0;
    uintptr_t base = UINTPTR_MAX;
    for (uint32_t i = 0; i < n; i++) {
        const debig_png_encode_desc *d = &descs[i];
        out_sizes[i] = 0;
        status[i] = DEBIG_PNG_E_ENCODE;
        if (!desc_ok(d) || !d_images[i] || ((uintptr_t)d_images[i] & ((1u << d->dtype) - 1u))) continue;
        status[i] = 0;
        enc_image *g = &im[n_good++];
        g->idx = i;
        g->stream_len = stream_bytes(d);
        g->stream_off = at;
        at = debig_align16(at + g->stream_len) + 16u;
        const uint64_t rb = g->stream_len / d->height - 1u;
        const uint64_t run = rb >= DEBIG_PNG_ENCODE_FILTER_BYTES ? 1u : DEBIG_PNG_ENCODE_FILTER_BYTES / rb;
        n_ft += (d->height + run - 1u) / run;
        g->first_task = n_dt;
        g->tasks = n_chunks(g->stream_len);
        n_dt += g->tasks;
        if ((uintptr_t)d_images[i] < base) base = (uintptr_t)d_images[i];
    }
    if (n_good == 0) {
        rc = 0;
        goto done;
    }
    if (n_ft >= 0x7fffffffu || n_dt >= 0x7fffffffu) goto done;
    /* the arena: the streams, the flags, the counts, then the slots; the files follow once their sizes are known */
    const uint64_t flags_off = at, counts_off = flags_off + debig_align16(4u * (uint64_t)n_good), slots_off = counts_off + debig_align16(4u * n_dt);
    const uint64_t blob_len = n_ft * 64u + n_dt * ts;
    blob = (uint8_t *)calloc((size_t)blob_len, 1);
    words = (uint32_t *)malloc((size_t)(n_good + n_dt) * 4u + 16u);
    if (!blob || !words) goto done;
    debig_png_encode_filter_task *ft = (debig_png_encode_filter_task *)blob;
    uint8_t *dt = blob + n_ft * 64u; /* deflate tasks, or dynamic / lz tasks at levels 2 / 3: ts bytes each */
    at = slots_off;
    for (uint32_t k = 0; k < n_good; k++) {
        const enc_image *g = &im[k];
        const debig_png_encode_desc *d = &descs[g->idx];
        const uint32_t rb = (uint32_t)(g->stream_len / d->height - 1u);
        const uint32_t run = rb >= DEBIG_PNG_ENCODE_FILTER_BYTES ? 1u : DEBIG_PNG_ENCODE_FILTER_BYTES / rb;
        for (uint32_t y0 = 0; y0 < d->height; y0 += run, ft++) {
            ft->image_off = (uint64_t)((uintptr_t)d_images[g->idx] - base);
            ft->stream_off = g->stream_off;
            ft->w = d->width;
            ft->h = d->height;
            ft->row0 = y0;
            ft->rows = d->height - y0 < run ? d->height - y0 : run;
            ft->channels = d->channels;
            ft->dtype = d->dtype;
            ft->depth = d->depth;
            ft->layout = d->layout;
            ft->filter = filter;
            ft->palette_entries = d->palette_entries;
            ft->flag_idx = k;
        }
        for (uint64_t j = 0; j < g->tasks; j++) {
            debig_png_encode_lz_task y; /* its first 64 bytes are the deflate task, all but row_stride the dynamic task */
            memset(&y, 0, sizeof y);
            y.stream_off = g->stream_off;
            y.stream_len = g->stream_len;
            y.chunk_off = j * DEBIG_PNG_ENCODE_CHUNK;
            y.chunk_len = (uint32_t)(g->stream_len - y.chunk_off < DEBIG_PNG_ENCODE_CHUNK ? g->stream_len - y.chunk_off : DEBIG_PNG_ENCODE_CHUNK);
            y.slot_off = at;
            y.slot_cap = (uint32_t)DEBIG_PNG_ENCODE_SLOT(y.chunk_len);
            y.level = level;
            y.bpp = d->channels * (d->depth / 8u);
            y.last = j + 1u == g->tasks;
            y.count_idx = (uint32_t)(g->first_task + j);
            y.token_off = ((g->first_task + j) % DEBIG_PNG_ENCODE_ROUND_TASKS) * TOKEN_ROW; /* the row of its place in its round */
            y.token_cap = (uint32_t)TOKEN_ROW;
            /* the byte above, where the rule takes it as a distance (a row of one pixel has S - bpp = 1: the rule skips it) */
            if (level == 3u && y.bpp < 1u + rb && 1u + rb + y.bpp <= 32768u) y.row_stride = 1u + rb;
            memcpy(dt + (g->first_task + j) * ts, &y, ts);
            at += y.slot_cap;
        }
    }
    const uint64_t files_off = at;
    /* ---- 2. .. 5. upload, the two launches, the counts and the flags ---- */
    debig_ctx *c = debig_ctx_get(0);
    if (!c) goto done;
    if ((rc = debig_devbuf_reserve(&c->rsz_tasks, blob_len)) || (rc = debig_devbuf_reserve(&c->rsz_weights, files_off)) ||
        (rc = debig_hip_memcpy_h2d(c->rsz_tasks.ptr, blob, blob_len, NULL)))
        goto done;
    uint8_t *arena = (uint8_t *)c->rsz_weights.ptr;
    const uint8_t *d_dt = (const uint8_t *)c->rsz_tasks.ptr + n_ft * 64u;
    if ((rc = debig_hip_memset(arena + flags_off, 0, slots_off - flags_off, NULL)) ||
        (rc = debig_hip_png_encode_filter_batch((const void *)base, arena, (const debig_png_encode_filter_task *)c->rsz_tasks.ptr,
                                                arena + flags_off, (uint32_t)n_ft, NULL)))
        goto done;
    if (level >= 2u) {
        /* rounds on one stream run one behind the other: a round's token rows are free when the next one starts */
        const uint64_t round = n_dt < DEBIG_PNG_ENCODE_ROUND_TASKS ? n_dt : DEBIG_PNG_ENCODE_ROUND_TASKS;
        if ((rc = debig_devbuf_reserve(&c->enc_tokens, round * TOKEN_ROW))) goto done;
        for (uint64_t r0 = 0; r0 < n_dt; r0 += round) {
            const uint64_t m = n_dt - r0 < round ? n_dt - r0 : round;
            if (level == 3u)
                rc = debig_hip_png_encode_lz_batch(arena, arena, c->enc_tokens.ptr, (const debig_png_encode_lz_task *)(d_dt + r0 * ts), arena + counts_off,
                                                   (uint32_t)m, NULL);
            else
                rc = debig_hip_png_encode_dynamic_batch(arena, arena, c->enc_tokens.ptr, (const debig_png_encode_dynamic_task *)(d_dt + r0 * ts),
                                                        arena + counts_off, (uint32_t)m, NULL);
            if (rc) goto done;
        }
    } else if ((rc = debig_hip_png_encode_deflate_batch(arena, arena, (const debig_png_encode_deflate_task *)d_dt, arena + counts_off, (uint32_t)n_dt,
                                                        NULL)))
        goto done;
    if ((rc = debig_hip_memcpy_d2h(words, arena + flags_off, 4u * (uint64_t)n_good, NULL)) ||
        (rc = debig_hip_memcpy_d2h(words + n_good, arena + counts_off, 4u * n_dt, NULL)) || (rc = debig_hip_stream_sync(NULL)))
        goto done;
    /* ---- 6. the files: sizes, statuses, places; what the host writes and the copy list ---- */
    uint32_t n_files = 0;
    uint64_t heads_len = 0, n_copies = 0;
    at = 0;
    for (uint32_t k = 0; k < n_good; k++) {
        enc_image *g = &im[k];
        const debig_png_encode_desc *d = &descs[g->idx];
        if (words[k]) {
            status[g->idx] = DEBIG_PNG_E_RANGE;
            continue;
        }
        for (uint64_t j = 0; j < g->tasks; j++) g->deflate_bytes += words[n_good + g->first_task + j];
        g->file_size = head_bytes(d) + 12u + 2u + g->deflate_bytes + 4u + 12u;
        if (g->file_size > debig_png_encode_bound(d)) { /* (a task that was skipped or wrote too much: never) */
            rc = 2;
            goto done;
        }
        if (!outs[g->idx] || out_caps[g->idx] < g->file_size) {
            status[g->idx] = DEBIG_PNG_E_OUTPUT;
            out_sizes[g->idx] = g->file_size;
            g->file_size = 0;
            continue;
        }
        g->file_off = at;
        at = debig_align16(at + g->file_size) + 16u;
        g->head_off = heads_len;
        heads_len = debig_align16(heads_len + head_bytes(d) + 10u + 16u);
        n_copies += 2u + g->tasks;
        n_files++;
    }
    if (n_files == 0) {
        rc = 0;
        goto done;
    }
    /* behind the files in the arena: the host's bytes, the copy list, the spans, the checksum words */
    const uint64_t heads_off = files_off + at, copies_off = heads_off + heads_len, spans_off = copies_off + n_copies * sizeof(debig_copy);
    const uint64_t sums_off = spans_off + 2u * (uint64_t)n_files * sizeof(debig_span), arena_len = sums_off + 8u * (uint64_t)n_files + 16u;
    heads = (uint8_t *)calloc((size_t)heads_len, 1);
    copies = (debig_copy *)calloc((size_t)n_copies, sizeof *copies);
    spans = (debig_span *)calloc(2u * (size_t)n_files, sizeof *spans);
    if (!heads || !copies || !spans) {
        rc = 2;
        goto done;
    }
    /* (the streams and the slots in the arena must survive: the files get a buffer of their own) */
    if ((rc = debig_devbuf_reserve(&c->files, arena_len - files_off))) goto done;
    uint8_t *farena = (uint8_t *)c->files.ptr; /* offsets rel. to files_off from here on */
    debig_copy *cp = copies;
    uint32_t f = 0;
    for (uint32_t k = 0; k < n_good; k++) {
        const enc_image *g = &im[k];
        const debig_png_encode_desc *d = &descs[g->idx];
        if (status[g->idx] || !g->file_size) continue;
        uint8_t *h = heads + g->head_off, ihdr[13];
        size_t hl = 8;
        memcpy(h, png_sig, 8);
        be32(ihdr, d->width);
        be32(ihdr + 4, d->height);
        ihdr[8] = (uint8_t)d->depth;
        ihdr[9] = d->palette_entries ? 3u : d->channels == 1u ? 0u : d->channels == 2u ? 4u : d->channels == 3u ? 2u : 6u;
        ihdr[10] = ihdr[11] = ihdr[12] = 0;
        hl += put_chunk(h + hl, "IHDR", ihdr, 13);
        if (d->palette_entries) hl += put_chunk(h + hl, "PLTE", side + d->palette_off, 3u * d->palette_entries);
        if (d->trns_entries) hl += put_chunk(h + hl, "tRNS", side + d->trns_off, d->trns_entries);
        be32(h + hl, (uint32_t)(2u + g->deflate_bytes + 4u));
        memcpy(h + hl + 4, "IDAT", 4);
        h[hl + 8] = 0x78;
        h[hl + 9] = level == 3u ? 0x9C : level == 2u ? 0x5E : 0x01; /* FLEVEL 0, 1 at level 2, 2 at level 3; FCHECK */
        hl += 10;
        /* the head, the chunk outputs, IEND (the Adler-32 and the IDAT's CRC-32 are patched in behind the checksum launches) */
        cp->src_off = (heads_off - files_off) + g->head_off;
        cp->dst_off = g->file_off;
        cp->len = hl;
        cp++;
        uint64_t to = g->file_off + hl;
        for (uint64_t j = 0; j < g->tasks; j++, cp++) {
            cp->src_off = task_slot_off(dt, ts, g->first_task + j);
            cp->dst_off = to;
            cp->len = words[n_good + g->first_task + j];
            to += cp->len;
        }
        uint8_t *iend = h + hl;
        put_chunk(iend, "IEND", NULL, 0);
        cp->src_off = (heads_off - files_off) + g->head_off + hl;
        cp->dst_off = to + 8u;
        cp->len = 12;
        cp++;
        spans[f].off = g->stream_off; /* Adler-32: the filtered stream */
        spans[f].len = g->stream_len;
        spans[n_files + f].off = g->file_off + hl - 6u; /* CRC-32: the IDAT's type and data, the Adler-32 included */
        spans[n_files + f].len = 4u + 2u + g->deflate_bytes + 4u;
        f++;
    }
    /* the first and the last copy of a file read the host's bytes in the files buffer, the others the slots in the arena: two lists */
    {
        debig_copy *own = (debig_copy *)malloc((size_t)(2u * n_files) * sizeof *own), *slot = (debig_copy *)malloc((size_t)(n_copies - 2u * n_files + 1u) * sizeof *slot);
        uint64_t n_own = 0, n_slot = 0;
        if (!own || !slot) {
            free(own);
            free(slot);
            rc = 2;
            goto done;
        }
        cp = copies;
        for (uint32_t k = 0; k < n_good; k++) {
            const enc_image *g = &im[k];
            if (status[g->idx] || !g->file_size) continue;
            own[n_own++] = *cp++;
            for (uint64_t j = 0; j < g->tasks; j++) slot[n_slot++] = *cp++;
            own[n_own++] = *cp++;
        }
        memcpy(copies, own, (size_t)n_own * sizeof *own);
        memcpy(copies + n_own, slot, (size_t)n_slot * sizeof *slot);
        free(own);
        free(slot);
        const uint64_t co = copies_off - files_off, so = spans_off - files_off, su = sums_off - files_off;
        uint32_t *sums = words; /* (the counts are in the copy list by now) */
        if ((rc = debig_hip_memcpy_h2d(farena + (heads_off - files_off), heads, heads_len, NULL)) ||
            (rc = debig_hip_memcpy_h2d(farena + co, copies, n_copies * sizeof *copies, NULL)) ||
            (rc = debig_hip_memcpy_h2d(farena + so, spans, 2u * (uint64_t)n_files * sizeof *spans, NULL)) ||
            (rc = debig_hip_gather(farena, farena, (const debig_copy *)(farena + co), (uint32_t)n_own, NULL)) ||
            (rc = debig_hip_gather(arena, farena, (const debig_copy *)(farena + co) + n_own, (uint32_t)n_slot, NULL)) ||
            /* ---- 7., 8. the Adler-32 of every stream into its file, then the CRC-32 of every IDAT ---- */
            (rc = debig_hip_checksum_batch(arena, (const debig_span *)(farena + so), (uint32_t *)(farena + su), n_files, 1u, NULL)) ||
            (rc = debig_hip_memcpy_d2h(sums, farena + su, 4u * (uint64_t)n_files, NULL)) || (rc = debig_hip_stream_sync(NULL)))
            goto done;
        for (f = 0; f < n_files; f++) { /* (the stream is idle: `heads` has been uploaded and is free to hold the four bytes per file) */
            uint8_t *a = heads + 4u * (size_t)f;
            be32(a, sums[f]);
            const uint64_t where = spans[n_files + f].off + spans[n_files + f].len - 4u;
            if ((rc = debig_hip_memcpy_h2d(farena + where, a, 4, NULL))) goto done;
        }
        if ((rc = debig_hip_checksum_batch(farena, (const debig_span *)(farena + so) + n_files, (uint32_t *)(farena + su) + n_files, n_files, 0u, NULL)) ||
            (rc = debig_hip_memcpy_d2h(sums, farena + su + 4u * (uint64_t)n_files, 4u * (uint64_t)n_files, NULL)))
            goto done;
        /* ---- 9. every good file once; its CRC word arrives with the sums and is written into the host copy ---- */
        for (uint32_t k = 0; k < n_good; k++) {
            const enc_image *g = &im[k];
            if (status[g->idx] || !g->file_size) continue;
            if ((rc = debig_hip_memcpy_d2h(outs[g->idx], farena + g->file_off, g->file_size, NULL))) goto done;
        }
        if ((rc = debig_hip_stream_sync(NULL))) goto done;
        f = 0;
        for (uint32_t k = 0; k < n_good; k++) {
            const enc_image *g = &im[k];
            if (status[g->idx] || !g->file_size) continue;
            be32((uint8_t *)outs[g->idx] + g->file_size - 16u, sums[f++]);
            out_sizes[g->idx] = g->file_size;
        }
    }
    rc = 0;
done:
    if (rc)
        for (uint32_t i = 0; i < n; i++) out_sizes[i] = 0;
    free(im);
    free(blob);
    free(heads);
    free(words);
    free(copies);
    free(spans);
    return rc;
}

DEBIG_API int debig_png_encode_batch(const void *const *d_images, const debig_png_encode_desc *descs, const uint8_t *side, void *const *outs,
                                     const uint64_t *out_caps, uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter,
                                     uint32_t level)
{
    if (n == 0) return 0;
    if (!args_ok(d_images, descs, side, outs, out_caps, out_sizes, status, n, filter, level, 1u)) return DEBIG_PNG_BAD_ARG;
    return encode_body(d_images, descs, side, outs, out_caps, out_sizes, status, n, filter, level);
}

DEBIG_API int debig_png_encode_batch_dyn(const void *const *d_images, const debig_png_encode_desc *descs, const uint8_t *side, void *const *outs,
                                         const uint64_t *out_caps, uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter,
                                         uint32_t level)
{
    if (n == 0) return 0;
    if (!args_ok(d_images, descs, side, outs, out_caps, out_sizes, status, n, filter, level, 2u)) return DEBIG_PNG_BAD_ARG;
    return encode_body(d_images, descs, side, outs, out_caps, out_sizes, status, n, filter, level);
}

DEBIG_API int debig_png_encode_batch_lz(const void *const *d_images, const debig_png_encode_desc *descs, const uint8_t *side, void *const *outs,
                                        const uint64_t *out_caps, uint64_t *out_sizes, uint32_t *status, uint32_t n, uint32_t filter,
                                        uint32_t level)
{
    if (n == 0) return 0;
    if (!args_ok(d_images, descs, side, outs, out_caps, out_sizes, status, n, filter, level, 3u)) return DEBIG_PNG_BAD_ARG;
    return encode_body(d_images, descs, side, outs, out_caps, out_sizes, status, n, filter, level);
}
