/*
 * debig_png_info_get / debig_png_decode_batch / debig_png_decode_batch_fmt / debig_png_out_layout (include/decode_png.h):
 * every PNG the specification allows, to RGBA8 or to the output format the caller asks for.  Not a reference function.
 * debig_png_decode_batch_tensor (towards the end of the file): the same decode into the context's own device arena, then one
 * resize + normalise launch (debig_hip_png_resize_batch) into the caller's dense tensor.
 * debig_png_decode_batch_labels (at the end of the file): palette indices and raw grey samples into that arena
 * (debig_hip_png_spec_defilter_index_batch), then one crop + nearest + remap + widen launch (debig_hip_png_label_gather_batch).
 * debig_png_decode_batch_color_labels (after it): RGB8 into that arena, then one crop + nearest + pack + colour lookup + widen
 * launch (debig_hip_png_color_label_batch).  These three share one staging path (stage_decode: IHDR rules, box, arena place,
 * decode) and one way to the device (dev_tables_place, dev_upload), between the tensor call's checks and its core.
 *
 * Host side (plain C): the chunk walk and the rules decided by headers alone.  On the GPU: chunk CRC-32 and the
 * Adler-32 trailer (debig_hip_checksum_batch), the IDAT concatenation (debig_hip_gather), inflate (the batch inflate,
 * plain RFC 1951) and the de-filter -- the tuned kernels for non-interlaced 8-bit RGB / RGBA to RGBA8, the general
 * kernel (debig_hip_png_spec_defilter_batch: every colour type, depth, Adam7 pass, tRNS) for the rest of RGBA8, and
 * its output-format twin (debig_hip_png_spec_defilter_fmt_batch) for every image whose resolved format is not RGBA8.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "decode_png.h"
#include "debig_ctx.h"
#include "debig_png_spec.h"

static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
static const uint32_t adam7[7][4] = {{0, 0, 8, 8}, {4, 0, 8, 8}, {0, 4, 4, 8}, {2, 0, 4, 4}, {0, 2, 2, 4}, {1, 0, 2, 2}, {0, 1, 1, 2}};

static uint32_t sbe32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

static uint32_t channels_of(uint32_t ct) { return ct == 0 ? 1u : ct == 2 ? 3u : ct == 3 ? 1u : ct == 4 ? 2u : 4u; }
static int depth_ok(uint32_t ct, uint32_t d)
{
    switch (ct) {
    case 0: return d == 1 || d == 2 || d == 4 || d == 8 || d == 16;
    case 3: return d == 1 || d == 2 || d == 4 || d == 8;
    case 2: case 4: case 6: return d == 8 || d == 16;
    default: return 0;
    }
}

/* pass p of a w x h image (interlace 0: p = 0 is the whole image) */
static void pass_dims(uint32_t w, uint32_t h, uint32_t il, uint32_t p, uint32_t g[4], uint32_t *wp, uint32_t *hp)
{
    static const uint32_t whole[4] = {0, 0, 1, 1};
    const uint32_t *q = il ? adam7[p] : whole;
    memcpy(g, q, 4 * sizeof(uint32_t));
    *wp = w > q[0] ? (w - q[0] + q[2] - 1) / q[2] : 0;
    *hp = h > q[1] ? (h - q[1] + q[3] - 1) / q[3] : 0;
}
static uint64_t row_bytes(uint64_t wp, uint32_t ct, uint32_t depth) { return (wp * channels_of(ct) * depth + 7u) / 8u; }

static int grow(void **p, uint32_t *cap, uint32_t n, size_t elem)
{
    if (n < *cap) return 1;
    uint32_t c = *cap ? 2 * *cap : 16;
    void *q = realloc(*p, (size_t)c * elem);
    if (!q) return 0;
    *p = q;
    *cap = c;
    return 1;
}
int spec_grow(void **p, uint32_t *cap, uint32_t n, size_t elem) { return grow(p, cap, n, elem); }
uint32_t spec_be32(const uint8_t *p) { return sbe32(p); }

int spec_zlib_header_ok(uint32_t cmf, uint32_t flg)
{
    return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) | flg) % 31u == 0u && !(flg & 0x20u);
}

uint64_t spec_scan_bytes(const debig_png_info *info, uint32_t w, uint32_t h)
{
    const uint32_t ct = info->color_type, d = info->bit_depth, il = info->interlace;
    uint64_t scan = 0;
    for (uint32_t p = 0; p < (il ? 7u : 1u); p++) {
        uint32_t g[4], wp, hp;
        pass_dims(w, h, il, p, g, &wp, &hp);
        if (wp && hp) scan += (uint64_t)hp * (1u + row_bytes(wp, ct, d));
    }
    return scan;
}

int spec_is_general(const spec_file *F, uint32_t flags)
{
    const uint32_t ct = F->info.color_type, d = F->info.bit_depth, il = F->info.interlace;
    return (flags & DEBIG_PNG_FORCE_GENERAL) || F->fmt || F->planar || il || d != 8 || !(ct == 6 || (ct == 2 && !F->has_key));
}

uint64_t spec_general_scratch(const debig_png_info *info, uint32_t w, uint32_t h, uint32_t *n_tasks)
{
    const uint32_t ct = info->color_type, d = info->bit_depth, il = info->interlace;
    uint64_t bytes = 0;
    *n_tasks = 0;
    for (uint32_t p = 0; p < (il ? 7u : 1u); p++) {
        uint32_t g[4], wp, hp;
        pass_dims(w, h, il, p, g, &wp, &hp);
        if (!wp || !hp) continue;
        bytes += DEBIG_PNG_SPEC_SCRATCH_BYTES(row_bytes(wp, ct, d));
        (*n_tasks)++;
    }
    return bytes;
}

uint32_t spec_image_tasks(const spec_file *F, uint32_t w, uint32_t h, uint64_t stream_off, uint64_t rgba_off,
                          uint64_t scratch_off, debig_png_spec_task *tasks)
{
    const uint32_t ct = F->info.color_type, d = F->info.bit_depth, il = F->info.interlace;
    uint64_t pos = stream_off, scratch = scratch_off;
    uint32_t n = 0;
    for (uint32_t p = 0; p < (il ? 7u : 1u); p++) {
        uint32_t g[4], wp, hp;
        pass_dims(w, h, il, p, g, &wp, &hp);
        if (!wp || !hp) continue;
        const uint64_t rb = row_bytes(wp, ct, d);
        debig_png_spec_task *t = &tasks[n++];
        t->stream_off = pos;
        t->rgba_off = rgba_off;
        t->pal_off = F->pal_off;
        t->scratch_off = scratch;
        t->width = wp;
        t->height = hp;
        t->img_width = w;
        t->img_height = h;
        t->x0 = g[0]; t->y0 = g[1]; t->dx = g[2]; t->dy = g[3];
        t->depth = (uint8_t)d;
        t->color_type = (uint8_t)ct;
        t->channels = (uint8_t)channels_of(ct);
        t->bpp_f = (uint8_t)(t->channels * d / 8u ? t->channels * d / 8u : 1u);
        memcpy(t->key, F->key, sizeof t->key);
        t->has_key = (uint16_t)F->has_key;
        t->n_pal = (uint16_t)F->n_pal;
        t->out_fmt = (uint16_t)F->fmt;
        pos += (uint64_t)hp * (1u + rb);
        scratch += DEBIG_PNG_SPEC_SCRATCH_BYTES(rb);
    }
    return n;
}

/* byte k of the IDAT concatenation (k < z_total) */
static uint8_t z_byte(const spec_file *F, const uint8_t *in, uint64_t k)
{
    for (uint32_t i = 0; i < F->n_idat; i++) {
        if (k < F->idat[i].len) return in[F->idat[i].off + k];
        k -= F->idat[i].len;
    }
    return 0;
}

/* The chunk walk.  info_only: stop at the first IDAT (debig_png_info_get).  Returns a DEBIG_PNG_* status. */
uint32_t spec_walk(const uint8_t *in, uint64_t size, spec_file *F, int info_only)
{
    if (!in || size < 8 || memcmp(in, png_sig, 8)) return DEBIG_PNG_E_SIGNATURE;
    uint64_t pos = 8;
    int seen_ihdr = 0, seen_plte = 0, seen_idat = 0, idat_done = 0, have_pal = 0;
    int64_t trns_at = -1;
    uint32_t trns_len = 0;
    int trns_after_plte = 0;
    for (;;) {
        if (pos + 8 > size) return DEBIG_PNG_E_CHUNK;
        const uint32_t len = sbe32(in + pos);
        const uint8_t *type = in + pos + 4;
        if (len > 0x7fffffffu || pos + 12 + (uint64_t)len > size) return DEBIG_PNG_E_CHUNK;
        const uint8_t *body = in + pos + 8;
        if (!seen_ihdr && memcmp(type, "IHDR", 4)) return DEBIG_PNG_E_CHUNK;
        int is_iend = 0;
        if (!memcmp(type, "IHDR", 4)) {
            if (seen_ihdr) return DEBIG_PNG_E_CHUNK;
            if (len != 13) return DEBIG_PNG_E_IHDR;
            const uint32_t w = sbe32(body), h = sbe32(body + 4);
            const uint32_t d = body[8], ct = body[9];
            if (w < 1 || w > 0x7fffffffu || h < 1 || h > 0x7fffffffu || !depth_ok(ct, d) || body[10] || body[11] || body[12] > 1)
                return DEBIG_PNG_E_IHDR;
            F->info.width = w;
            F->info.height = h;
            F->info.bit_depth = (uint8_t)d;
            F->info.color_type = (uint8_t)ct;
            F->info.interlace = body[12];
            seen_ihdr = 1;
        } else if (!memcmp(type, "IDAT", 4)) {
            if (idat_done) return DEBIG_PNG_E_CHUNK;
            if (info_only) break;
            seen_idat = 1;
            if (len) {
                if (!grow((void **)&F->idat, &F->cap_idat, F->n_idat, sizeof(spec_piece))) return DEBIG_PNG_E_CHUNK;
                F->idat[F->n_idat].off = pos + 8;
                F->idat[F->n_idat].len = len;
                F->n_idat++;
                F->z_total += len;
            }
        } else {
            if (seen_idat) idat_done = 1;
            const uint32_t ct = F->info.color_type;
            if (!memcmp(type, "IEND", 4)) {
                is_iend = 1;
            } else if (!memcmp(type, "PLTE", 4)) {
                if (seen_plte || seen_idat || ct == 0 || ct == 4) return DEBIG_PNG_E_CHUNK;
                seen_plte = 1;
                if (ct == 3) {
                    if (len % 3u || len < 3 || len > 768) return DEBIG_PNG_E_PALETTE;
                    F->n_pal = len / 3u;
                    for (uint32_t k = 0; k < F->n_pal; k++)
                        F->pal[k] = (uint32_t)body[3 * k] | ((uint32_t)body[3 * k + 1] << 8) | ((uint32_t)body[3 * k + 2] << 16) | 0xff000000u;
                    have_pal = 1;
                }
            } else if (!memcmp(type, "tRNS", 4)) {
                if (!seen_idat) {
                    trns_at = (int64_t)(pos + 8);
                    trns_len = len;
                    trns_after_plte = have_pal;
                }
            } else if (!(type[0] & 0x20u)) {
                return DEBIG_PNG_E_CHUNK; /* unknown critical chunk */
            }
        }
        if (!info_only) {
            if (!grow((void **)&F->chunks, &F->cap_chunks, F->n_chunks, sizeof(spec_chunk))) return DEBIG_PNG_E_CHUNK;
            F->chunks[F->n_chunks].off = pos + 4;
            F->chunks[F->n_chunks].len = (uint64_t)len + 4u;
            F->chunks[F->n_chunks].crc = sbe32(body + len);
            F->n_chunks++;
        }
        pos += 12 + (uint64_t)len;
        if (is_iend) break;
    }
    const uint32_t ct = F->info.color_type;
    if (ct == 3 && !have_pal) return DEBIG_PNG_E_CHUNK;
    if (trns_at >= 0) {
        const uint8_t *b = in + trns_at;
        if (ct == 3 && trns_after_plte && trns_len <= F->n_pal) {
            for (uint32_t k = 0; k < trns_len; k++) F->pal[k] = (F->pal[k] & 0x00ffffffu) | ((uint32_t)b[k] << 24);
            F->info.has_trns = 1;
        } else if (ct == 0 && trns_len == 2) {
            F->key[0] = (uint16_t)((b[0] << 8) | b[1]);
            F->has_key = F->info.has_trns = 1;
        } else if (ct == 2 && trns_len == 6) {
            for (int k = 0; k < 3; k++) F->key[k] = (uint16_t)((b[2 * k] << 8) | b[2 * k + 1]);
            F->has_key = F->info.has_trns = 1;
        }
    }
    if (info_only) return DEBIG_PNG_OK;
    if (!seen_idat) return DEBIG_PNG_E_CHUNK;
    return DEBIG_PNG_OK;
}

void spec_free(spec_file *F)
{
    free(F->chunks);
    free(F->idat);
    F->chunks = NULL;
    F->idat = NULL;
}

DEBIG_API uint32_t debig_png_info_get(const uint8_t *p, uint64_t size, debig_png_info *info)
{
    spec_file F;
    memset(&F, 0, sizeof F);
    const uint32_t st = spec_walk(p, size, &F, 1);
    if (info) *info = F.info;
    spec_free(&F);
    return st;
}

static int fmt_valid(uint32_t f) { return (f & ~0x3fu) == 0 && (f & 15u) <= DEBIG_PNG_FMT_NATIVE && (f & 0x30u) != 0x30u; }

/* out_format -> the concrete layout (0..3) | DEBIG_PNG_FMT_16 of one image (out_format valid, info from the walk) */
static uint32_t fmt_resolve(const debig_png_info *info, uint32_t out_format)
{
    uint32_t lay = out_format & 15u, d16 = out_format & 0x30u;
    const uint32_t ct = info->color_type;
    if (lay == DEBIG_PNG_FMT_NATIVE) {
        if (ct == 0) lay = info->has_trns ? DEBIG_PNG_FMT_GRAY_ALPHA : DEBIG_PNG_FMT_GRAY;
        else if (ct == 4) lay = DEBIG_PNG_FMT_GRAY_ALPHA;
        else if (ct == 2 || ct == 3) lay = info->has_trns ? DEBIG_PNG_FMT_RGBA : DEBIG_PNG_FMT_RGB;
        else lay = DEBIG_PNG_FMT_RGBA;
    }
    if (d16 == DEBIG_PNG_FMT_NATIVE_DEPTH) d16 = info->bit_depth == 16 ? DEBIG_PNG_FMT_16 : DEBIG_PNG_FMT_8;
    return lay | d16;
}
static uint32_t fmt_channels(uint32_t fmt) { const uint32_t l = fmt & 15u; return l == 0 ? 4u : l == 1 ? 3u : l == 2 ? 1u : 2u; }
/* w * h * bytes per pixel (w, h < 2^31), UINT64_MAX where that does not fit 64 bits */
static uint64_t fmt_size(uint64_t w, uint64_t h, uint32_t fmt)
{
    const uint64_t wh = w * h, pb = (uint64_t)fmt_channels(fmt) * (fmt & DEBIG_PNG_FMT_16 ? 2u : 1u);
    return wh > UINT64_MAX / pb ? UINT64_MAX : wh * pb;
}

DEBIG_API uint64_t debig_png_out_layout(const debig_png_info *info, uint32_t out_format, uint32_t *channels,
                                        uint32_t *bytes_per_sample)
{
    if (!info || !fmt_valid(out_format) || !depth_ok(info->color_type, info->bit_depth)) return 0;
    const uint32_t f = fmt_resolve(info, out_format), ch = fmt_channels(f), bs = f & DEBIG_PNG_FMT_16 ? 2u : 1u;
    if (channels) *channels = ch;
    if (bytes_per_sample) *bytes_per_sample = bs;
    return fmt_size(info->width, info->height, f);
}

/* the host rules after the walk: zlib header, output size; and the sizes the device needs */
static uint32_t spec_host_rules(spec_file *F, const uint8_t *in, int have_out, uint64_t out_cap, uint32_t out_format)
{
    if (F->z_total < 2) return DEBIG_PNG_E_ZLIB;
    if (!spec_zlib_header_ok(z_byte(F, in, 0), z_byte(F, in, 1))) return DEBIG_PNG_E_ZLIB;
    const uint64_t w = F->info.width, h = F->info.height;
    F->fmt = fmt_resolve(&F->info, out_format);
    F->out_bytes = fmt_size(w, h, F->fmt); /* UINT64_MAX (no buffer that large): E_OUTPUT */
    if (!have_out || out_cap < F->out_bytes) return DEBIG_PNG_E_OUTPUT;
    F->scan = spec_scan_bytes(&F->info, (uint32_t)w, (uint32_t)h);
    return DEBIG_PNG_OK;
}

DEBIG_API int debig_png_decode_batch(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                                     const uint64_t *out_caps, uint32_t *status, debig_png_info *infos, uint32_t n,
                                     uint32_t flags)
{
    return debig_png_decode_batch_fmt(inputs, input_sizes, outs, out_caps, status, infos, n, flags, 0);
}

/* where the pixels go: host buffers (outs), or image i stays on the device at d_arena + d_offs[i] (outs NULL) */
typedef struct spec_target {
    uint8_t *const *outs;
    void *d_arena;
    const uint64_t *d_offs;
    uint64_t own_bytes;        /* != 0: the arena is the context's own (c->rsz_src, reserved here to own_bytes), d_arena unused */
    const uint32_t *pre_status; /* may be NULL; pre_status[i] != 0: file i ends with that status once its walk has filled info */
    uint32_t labels;           /* != 0 (debig_png_decode_batch_labels): every file through the raw-label de-filter kernel */
} spec_target;

typedef int (*spec_launch_fn)(void *, void *, const debig_png_spec_task *, debig_png_spec_result *, uint32_t, void *);

/* the decode behind debig_png_decode_batch_fmt / _layout / _dev and, through stage_decode, behind _tensor / _tensor_alpha /
 * _tensor_filter / _labels / _color_labels (out_format and out_layout valid) */
static int spec_decode_core(const uint8_t *const *inputs, const uint64_t *input_sizes, const spec_target *tg,
                            const uint64_t *out_caps, uint32_t *status, debig_png_info *infos, uint32_t n, uint32_t flags,
                            uint32_t out_format, uint32_t out_layout)
{
    if (n == 0) return 0;
    spec_file *F = (spec_file *)calloc(n, sizeof(spec_file));
    uint32_t *live = (uint32_t *)calloc(n, sizeof(uint32_t)); /* files still good, in order */
    debig_span *spans = NULL;
    uint32_t *sums = NULL;
    debig_copy *copies = NULL;
    debig_stream *desc = NULL;
    debig_result *res = NULL;
    debig_png_image *img = NULL;
    debig_png_result *ires = NULL;
    debig_png_spec_task *tasks = NULL;
    debig_png_spec_result *tres = NULL;
    uint32_t *task_file = NULL, *img_file = NULL;
    uint8_t **dn_dst = NULL;
    uint64_t *dn_size = NULL, *dn_off = NULL, *up_size = NULL, *up_off = NULL;
    int rc = 2;
    if (!F || !live) goto done;
    rc = 0;
    /* ---- host rules */
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
        spec_file *f = &F[i];
        f->status = spec_walk(inputs[i], input_sizes[i], f, 0);
        if (tg->pre_status && tg->pre_status[i])
            f->status = tg->pre_status[i];
        else if (f->status == DEBIG_PNG_OK)
            f->status = spec_host_rules(f, inputs[i], tg->outs ? tg->outs[i] != NULL : 1, out_caps[i], out_format);
        if (f->status == DEBIG_PNG_OK) {
            f->planar = out_layout == DEBIG_PNG_LAYOUT_CHW && fmt_channels(f->fmt) > 1u; /* one channel: the same bytes */
            live[m++] = i;
        }
    }
    if (m == 0) goto report; /* nothing for the device */
    debig_ctx *c = debig_ctx_get(0);
    if (!c) { rc = 1; goto done; }
    /* ---- device layout: whole files (c->files); IDAT concatenations (c->in); per file in c->out the scanline stream
     *      (+ 16 readable bytes), the palette and the scratch rings of its general-kernel tasks; pixels (c->rgba, each
     *      image 16-byte aligned), or the caller's device arena */
    uint64_t files_total = 0, in_total = 0, out_total = 64, rgba_total = 0;
    uint32_t n_chunks = 0, n_pieces = 0, n_tasks = 0, n_img = 0, cnt[4] = {0, 0, 0, 0}; /* cnt: tasks per de-filter kernel */
    for (uint32_t k = 0; k < m; k++) {
        spec_file *f = &F[live[k]];
        const uint32_t ct = f->info.color_type;
        f->general = tg->labels || spec_is_general(f, flags);
        f->file_off = files_total;
        files_total += debig_align16(input_sizes[live[k]]) + 16;
        f->in_off = in_total;
        in_total += debig_align16(f->z_total) + 32;
        f->out_off = out_total;
        out_total += debig_align16(f->scan) + 32;
        f->pal_off = out_total;
        if (ct == 3) out_total += 1024;
        f->scratch_off = out_total;
        f->rgba_off = tg->outs ? rgba_total : tg->d_offs[live[k]];
        rgba_total += debig_align16(f->out_bytes) + 16;
        n_chunks += f->n_chunks;
        n_pieces += f->n_idat;
        if (f->general) {
            uint32_t nt;
            out_total += spec_general_scratch(&f->info, f->info.width, f->info.height, &nt);
            n_tasks += nt;
            cnt[tg->labels ? 3 : f->planar ? 2 : f->fmt ? 1 : 0] += nt;
        } else {
            n_img++;
        }
    }
    spans = (debig_span *)calloc((size_t)n_chunks + m, sizeof(debig_span));
    sums = (uint32_t *)calloc((size_t)n_chunks + m, sizeof(uint32_t));
    copies = (debig_copy *)calloc((size_t)n_pieces + 1, sizeof(debig_copy));
    desc = (debig_stream *)calloc(m, sizeof(debig_stream));
    res = (debig_result *)calloc(m, sizeof(debig_result));
    img = (debig_png_image *)calloc((size_t)n_img + 1, sizeof(debig_png_image));
    ires = (debig_png_result *)calloc((size_t)n_img + 1, sizeof(debig_png_result));
    img_file = (uint32_t *)calloc((size_t)n_img + 1, sizeof(uint32_t));
    tasks = (debig_png_spec_task *)calloc((size_t)n_tasks + 1, sizeof(debig_png_spec_task));
    tres = (debig_png_spec_result *)calloc((size_t)n_tasks + 1, sizeof(debig_png_spec_result));
    task_file = (uint32_t *)calloc((size_t)n_tasks + 1, sizeof(uint32_t));
    up_size = (uint64_t *)calloc(n, sizeof(uint64_t));
    up_off = (uint64_t *)calloc(n, sizeof(uint64_t));
    dn_dst = (uint8_t **)calloc(n, sizeof(uint8_t *));
    dn_size = (uint64_t *)calloc(n, sizeof(uint64_t));
    dn_off = (uint64_t *)calloc(n, sizeof(uint64_t));
    if (!spans || !sums || !copies || !desc || !res || !img || !ires || !img_file || !tasks || !tres || !task_file ||
        !up_size || !up_off || !dn_dst || !dn_size || !dn_off) {
        rc = 2;
        goto done;
    }
    if ((rc = debig_devbuf_reserve(&c->files, files_total + 64)) || (rc = debig_devbuf_reserve(&c->in, in_total + 64)) ||
        (rc = debig_devbuf_reserve(&c->out, out_total + 64)) || (tg->outs && (rc = debig_devbuf_reserve(&c->rgba, rgba_total + 64))) ||
        (tg->own_bytes && (rc = debig_devbuf_reserve(&c->rsz_src, tg->own_bytes))) ||
        (rc = debig_devbuf_reserve(&c->spans, ((uint64_t)n_chunks + m) * sizeof(debig_span))) ||
        (rc = debig_devbuf_reserve(&c->crcs, ((uint64_t)n_chunks + m) * sizeof(uint32_t))) ||
        (rc = debig_devbuf_reserve(&c->copies, ((uint64_t)n_pieces + 1) * sizeof(debig_copy))))
        goto done;
    /* ---- whole files up; chunk CRCs and the IDAT concatenation on the device */
    for (uint32_t k = 0; k < m; k++) {
        up_size[live[k]] = input_sizes[live[k]];
        up_off[live[k]] = F[live[k]].file_off;
    }
    if ((rc = debig_upload_packed(c, c->files.ptr, inputs, up_size, up_off, n, files_total))) goto done;
    {
        uint32_t ci = 0, pi = 0;
        for (uint32_t k = 0; k < m; k++) {
            spec_file *f = &F[live[k]];
            for (uint32_t j = 0; j < f->n_chunks; j++, ci++) {
                spans[ci].off = f->file_off + f->chunks[j].off;
                spans[ci].len = f->chunks[j].len;
            }
            uint64_t dst = f->in_off;
            for (uint32_t j = 0; j < f->n_idat; j++, pi++) {
                copies[pi].src_off = f->file_off + f->idat[j].off;
                copies[pi].dst_off = dst;
                copies[pi].len = f->idat[j].len;
                dst += f->idat[j].len;
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
            spec_file *f = &F[live[k]];
            for (uint32_t j = 0; j < f->n_chunks; j++, ci++)
                if (f->status == DEBIG_PNG_OK && sums[ci] != f->chunks[j].crc) f->status = DEBIG_PNG_E_CRC;
        }
    }
    /* ---- inflate: plain RFC 1951 into exactly the scanline stream; the trailer and what follows stay in the span */
    uint32_t ns = 0;
    for (uint32_t k = 0; k < m; k++) {
        spec_file *f = &F[live[k]];
        if (f->status != DEBIG_PNG_OK) continue;
        live[ns] = live[k];
        desc[ns].in_off = f->in_off + 2u;
        desc[ns].in_len = f->z_total - 2u;
        desc[ns].out_off = f->out_off;
        desc[ns].out_cap = f->scan;
        desc[ns].flags = DEBIG_STREAM_NO_REF_GATES | DEBIG_STREAM_IMAGE_ROWS;
        ns++;
    }
    m = ns;
    if (m == 0) goto report;
    if ((rc = debig_launch_inflate_planned(c, c->in.ptr, desc, res, m))) goto done;
    ns = 0;
    for (uint32_t k = 0; k < m; k++) {
        spec_file *f = &F[live[k]];
        if (!res[k].good) {
            f->status = res[k].status == DEBIG_E_OUTPUT_FULL ? DEBIG_PNG_E_DATA_LONG : DEBIG_PNG_E_INFLATE;
            continue;
        }
        if (res[k].final_size < f->scan) { f->status = DEBIG_PNG_E_DATA_SHORT; continue; }
        const uint64_t t = 2u + (res[k].in_end_bits + 7u) / 8u; /* the Adler-32 trailer, in the concatenation */
        if (t + 4u > f->z_total) { f->status = DEBIG_PNG_E_ADLER; continue; }
        sums[ns] = ((uint32_t)z_byte(f, inputs[live[k]], t) << 24) | ((uint32_t)z_byte(f, inputs[live[k]], t + 1) << 16) |
                   ((uint32_t)z_byte(f, inputs[live[k]], t + 2) << 8) | z_byte(f, inputs[live[k]], t + 3);
        spans[ns].off = f->out_off;
        spans[ns].len = f->scan;
        live[ns++] = live[k];
    }
    m = ns;
    if (m == 0) goto report;
    {
        uint32_t *adl = sums + m; /* (sums holds n_chunks + m words, n_chunks >= 3 per file) */
        if ((rc = debig_hip_memcpy_h2d(c->spans.ptr, spans, (uint64_t)m * sizeof(debig_span), NULL)) ||
            (rc = debig_hip_checksum_batch(c->out.ptr, (const debig_span *)c->spans.ptr, (uint32_t *)c->crcs.ptr, m, 1, NULL)) ||
            (rc = debig_hip_memcpy_d2h(adl, c->crcs.ptr, (uint64_t)m * sizeof(uint32_t), NULL)) ||
            (rc = debig_hip_stream_sync(NULL)))
            goto done;
        ns = 0;
        for (uint32_t k = 0; k < m; k++) {
            if (adl[k] != sums[k]) { F[live[k]].status = DEBIG_PNG_E_ADLER; continue; }
            live[ns++] = live[k];
        }
        m = ns;
    }
    if (m == 0) goto report;
    /* ---- de-filter: tuned kernels for non-interlaced 8-bit RGB / RGBA to interleaved RGBA8; the general kernel for the
     *      rest of interleaved RGBA8 (tasks [0, cnt[0])), its output-format twin for every other interleaved format (the
     *      next cnt[1]) and the planar kernel for every channel-planar image of more than one channel (the next cnt[2]);
     *      in a label call every file is general and goes to the raw-label kernel (cnt[3], the other three empty) */
    static const spec_launch_fn launch[4] = {debig_hip_png_spec_defilter_batch, debig_hip_png_spec_defilter_fmt_batch,
                                             debig_hip_png_spec_defilter_planar_batch, debig_hip_png_spec_defilter_index_batch};
    void *pix = tg->outs ? c->rgba.ptr : tg->own_bytes ? c->rsz_src.ptr : tg->d_arena;
    const uint32_t base[4] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2]};
    uint32_t fill[4] = {0, 0, 0, 0};
    n_img = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = live[k];
        spec_file *f = &F[i];
        const uint32_t ct = f->info.color_type;
        if (!f->general) {
            debig_png_image *im = &img[n_img];
            im->stream_off = f->out_off;
            im->rgba_off = f->rgba_off;
            im->width = f->info.width;
            im->height = f->info.height;
            im->color_type = ct;
            img_file[n_img++] = i;
            continue;
        }
        if (ct == 3 && !tg->labels && (rc = debig_hip_memcpy_h2d((uint8_t *)c->out.ptr + f->pal_off, f->pal, 1024, NULL))) goto done;
        const uint32_t cls = tg->labels ? 3u : f->planar ? 2u : f->fmt ? 1u : 0u, t0 = base[cls] + fill[cls];
        const uint32_t nt = spec_image_tasks(f, f->info.width, f->info.height, f->out_off, f->rgba_off, f->scratch_off, &tasks[t0]);
        for (uint32_t j = 0; j < nt; j++) task_file[t0 + j] = i;
        fill[cls] += nt;
    }
    if (n_img) {
        if ((rc = debig_devbuf_reserve(&c->img, (uint64_t)n_img * sizeof(debig_png_image))) ||
            (rc = debig_devbuf_reserve(&c->imgres, (uint64_t)n_img * sizeof(debig_png_result))) ||
            (rc = debig_hip_memcpy_h2d(c->img.ptr, img, (uint64_t)n_img * sizeof(debig_png_image), NULL)) ||
            (rc = debig_hip_png_defilter_batch(c->out.ptr, pix, (const debig_png_image *)c->img.ptr,
                                               (debig_png_result *)c->imgres.ptr, n_img, NULL)) ||
            (rc = debig_hip_memcpy_d2h(ires, c->imgres.ptr, (uint64_t)n_img * sizeof(debig_png_result), NULL)))
            goto done;
    }
    if ((fill[0] || fill[1] || fill[2] || fill[3]) && /* the task lists in one buffer, reserved before any launch */
        ((rc = debig_devbuf_reserve(&c->spec_tasks, (uint64_t)(n_tasks + 1u) * sizeof(debig_png_spec_task))) ||
         (rc = debig_devbuf_reserve(&c->spec_res, (uint64_t)(n_tasks + 1u) * sizeof(debig_png_spec_result)))))
        goto done;
    for (uint32_t cls = 0; cls < 4; cls++) {
        if (!fill[cls]) continue;
        debig_png_spec_task *d_t = (debig_png_spec_task *)c->spec_tasks.ptr + base[cls];
        debig_png_spec_result *d_r = (debig_png_spec_result *)c->spec_res.ptr + base[cls];
        if ((rc = debig_hip_memcpy_h2d(d_t, tasks + base[cls], (uint64_t)fill[cls] * sizeof(debig_png_spec_task), NULL)) ||
            (rc = launch[cls](c->out.ptr, pix, d_t, d_r, fill[cls], NULL)) ||
            (rc = debig_hip_memcpy_d2h(tres + base[cls], d_r, (uint64_t)fill[cls] * sizeof(debig_png_spec_result), NULL)))
            goto done;
    }
    if ((rc = debig_hip_stream_sync(NULL))) goto done;
    for (uint32_t k = 0; k < n_img; k++)
        if (!ires[k].good) F[img_file[k]].status = DEBIG_PNG_E_FILTER;
    for (uint32_t cls = 0; cls < 4; cls++)
        for (uint32_t j = 0; j < fill[cls]; j++) { /* a filter error anywhere in the image outranks a palette error */
            const uint32_t k = base[cls] + j;
            spec_file *f = &F[task_file[k]];
            if (tres[k].status == DEBIG_PNG_SPEC_E_FILTER) f->status = DEBIG_PNG_E_FILTER;
            else if (tres[k].status == DEBIG_PNG_SPEC_E_PALETTE && f->status == DEBIG_PNG_OK) f->status = DEBIG_PNG_E_PALETTE;
        }
    /* ---- pixels down (host buffers only) */
    if (tg->outs) {
        uint64_t last_end = 0;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = live[k];
            if (F[i].status != DEBIG_PNG_OK) continue;
            dn_dst[i] = tg->outs[i];
            dn_size[i] = F[i].out_bytes;
            dn_off[i] = F[i].rgba_off;
            if (dn_off[i] + dn_size[i] > last_end) last_end = dn_off[i] + dn_size[i];
        }
        if (last_end && (rc = debig_download_unpack(c, c->rgba.ptr, dn_dst, dn_size, dn_off, n, last_end))) goto done;
    }
report:
    for (uint32_t i = 0; i < n; i++) {
        status[i] = F[i].status;
        if (infos) infos[i] = F[i].info;
    }
done:
    if (F)
        for (uint32_t i = 0; i < n; i++) spec_free(&F[i]);
    free(F);
    free(live);
    free(spans);
    free(sums);
    free(copies);
    free(desc);
    free(res);
    free(img);
    free(ires);
    free(img_file);
    free(tasks);
    free(tres);
    free(task_file);
    free(up_size);
    free(up_off);
    free(dn_dst);
    free(dn_size);
    free(dn_off);
    return rc;
}

DEBIG_API int debig_png_decode_batch_fmt(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                                         const uint64_t *out_caps, uint32_t *status, debig_png_info *infos, uint32_t n,
                                         uint32_t flags, uint32_t out_format)
{
    return debig_png_decode_batch_layout(inputs, input_sizes, outs, out_caps, status, infos, n, flags, out_format,
                                         DEBIG_PNG_LAYOUT_HWC);
}

DEBIG_API int debig_png_decode_batch_layout(const uint8_t *const *inputs, const uint64_t *input_sizes, uint8_t *const *outs,
                                            const uint64_t *out_caps, uint32_t *status, debig_png_info *infos, uint32_t n,
                                            uint32_t flags, uint32_t out_format, uint32_t out_layout)
{
    if (!fmt_valid(out_format) || out_layout > DEBIG_PNG_LAYOUT_CHW) return DEBIG_PNG_BAD_FORMAT;
    const spec_target tg = {outs, NULL, NULL, 0, NULL, 0};
    return spec_decode_core(inputs, input_sizes, &tg, out_caps, status, infos, n, flags, out_format, out_layout);
}

typedef struct spec_region { uint64_t off, cap; } spec_region;
static int by_off(const void *a, const void *b)
{
    const uint64_t x = ((const spec_region *)a)->off, y = ((const spec_region *)b)->off;
    return x < y ? -1 : x > y;
}

DEBIG_API int debig_png_decode_batch_dev(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out_arena,
                                         const uint64_t *out_offs, const uint64_t *out_caps, uint32_t *status,
                                         debig_png_info *infos, uint32_t n, uint32_t flags, uint32_t out_format,
                                         uint32_t out_layout)
{
    if (!fmt_valid(out_format) || out_layout > DEBIG_PNG_LAYOUT_CHW) return DEBIG_PNG_BAD_FORMAT;
    if (n == 0) return 0;
    /* the arguments on their own, before any file is looked at: arena, alignment, regions that do not overlap */
    if (!d_out_arena || !out_offs || !out_caps) return DEBIG_PNG_BAD_ARG;
    for (uint32_t i = 0; i < n; i++)
        if ((out_offs[i] & 15u) || out_offs[i] + out_caps[i] < out_offs[i]) return DEBIG_PNG_BAD_ARG;
    spec_region *reg = (spec_region *)malloc((size_t)n * sizeof(spec_region));
    if (!reg) return 2; /* out of host memory, the code the core returns for it */
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; i++)
        if (out_caps[i]) { /* an empty region overlaps nothing */
            reg[r].off = out_offs[i];
            reg[r++].cap = out_caps[i];
        }
    qsort(reg, r, sizeof(spec_region), by_off);
    int bad = 0;
    for (uint32_t k = 0; k + 1 < r; k++) bad |= reg[k].off + reg[k].cap > reg[k + 1].off;
    free(reg);
    if (bad) return DEBIG_PNG_BAD_ARG;
    const spec_target tg = {NULL, d_out_arena, out_offs, 0, NULL, 0};
    return spec_decode_core(inputs, input_sizes, &tg, out_caps, status, infos, n, flags, out_format, out_layout);
}

/* ---- debig_png_decode_batch_tensor: crop + resize + normalise into one dense device tensor (decode_png.h) ---------------- */

#define RSZ_MAX_TAPS 129u /* antialias is refused beyond a scale of 64: 2 * 64 + 1 taps */
#define RSZ_MAX_IMAGE_BYTES ((uint64_t)1 << 31)

DEBIG_API uint32_t debig_png_resize_weights(uint32_t cl, uint32_t L, uint32_t antialias, uint32_t X, uint32_t *first,
                                            int16_t *w, uint32_t w_cap)
{
    if (cl == 0 || L == 0 || L > 16384u || X >= L || !first || !w) return 0;
    const int64_t l2 = 2 * (int64_t)L;
    if (!antialias || cl <= L) {
        int64_t num = (2 * (int64_t)X + 1) * cl - L;
        const int64_t top = ((int64_t)cl - 1) * l2;
        num = num < 0 ? 0 : num > top ? top : num;
        const int64_t i0 = num / l2, r = num % l2, w1 = (r * 16384 + L) / l2;
        *first = (uint32_t)i0;
        if (i0 == (int64_t)cl - 1) {
            if (w_cap < 1) return 0;
            w[0] = 16384;
            return 1;
        }
        if (w_cap < 2) return 0;
        w[0] = (int16_t)(16384 - w1);
        w[1] = (int16_t)w1;
        return 2;
    }
    if ((uint64_t)cl > 64u * (uint64_t)L) return 0;
    const int64_t c = (2 * (int64_t)X + 1) * cl, reach = 2 * (int64_t)cl;
    int64_t j = c - reach > 0 ? (c - reach) / l2 : 0; /* (2j + 1) L <= c - 2 cl + L: at or left of the first tap */
    if (j > 0) j--;
#define RSZ_N(j) (reach - ((2 * (j) + 1) * (int64_t)L > c ? (2 * (j) + 1) * (int64_t)L - c : c - (2 * (j) + 1) * (int64_t)L))
    while (j < (int64_t)cl && RSZ_N(j) <= 0) j++;
    int64_t nn[RSZ_MAX_TAPS], T = 0, best = 0;
    uint32_t cnt = 0, best_k = 0;
    for (; j < (int64_t)cl && RSZ_N(j) > 0; j++) {
        if (cnt == RSZ_MAX_TAPS) return 0;
        if (cnt == 0) *first = (uint32_t)j;
        nn[cnt] = RSZ_N(j);
        T += nn[cnt];
        if (nn[cnt] > best) { best = nn[cnt]; best_k = cnt; }
        cnt++;
    }
#undef RSZ_N
    if (cnt == 0 || cnt > w_cap) return 0;
    int64_t sum = 0;
    for (uint32_t k = 0; k < cnt; k++) {
        const int64_t q = (nn[k] * 16384 + T / 2) / T;
        w[k] = (int16_t)q;
        sum += q;
    }
    w[best_k] = (int16_t)(w[best_k] + (16384 - sum));
    return cnt;
}

/* the Keys kernel (a = -1/2) times 2^29 at the distance m / D (decode_png.h: BICUBIC); m < 2 D */
static int64_t rsz_cubic_n(int64_t m, int64_t D)
{
    const int64_t u = (m * 65536) / D;
    const int64_t p = u <= 65536 ? 3 * u * u * u - 327680 * u * u + ((int64_t)1 << 49)
                                 : -u * u * u + 327680 * u * u - ((int64_t)1 << 35) * u + ((int64_t)1 << 50);
    return p >= 0 ? p >> 20 : -((-p + 1048575) >> 20); /* an arithmetic shift: floor(p / 2^20) */
}

DEBIG_API uint32_t debig_png_resize_weights_filter(uint32_t filter, uint32_t cl, uint32_t L, uint32_t antialias, uint32_t X,
                                                   uint32_t *first, int16_t *w, uint32_t w_cap)
{
    if (filter == DEBIG_PNG_FILTER_BILINEAR) return debig_png_resize_weights(cl, L, antialias, X, first, w, w_cap);
    if (cl == 0 || L == 0 || L > 16384u || X >= L || !first || !w) return 0;
    const int64_t l2 = 2 * (int64_t)L, c = (2 * (int64_t)X + 1) * cl;
    if (filter == DEBIG_PNG_FILTER_NEAREST) {
        if (w_cap < 1) return 0;
        *first = (uint32_t)(c / l2);
        w[0] = 16384;
        return 1;
    }
    if (filter != DEBIG_PNG_FILTER_BICUBIC) return 0;
    const int shrink = antialias && cl > L;
    if (shrink && (uint64_t)cl > 32u * (uint64_t)L) return 0;
    const int64_t D = shrink ? 2 * (int64_t)cl : l2, reach = 2 * D;
#define RSZ_M(j) ((2 * (j) + 1) * (int64_t)L > c ? (2 * (j) + 1) * (int64_t)L - c : c - (2 * (j) + 1) * (int64_t)L)
    int64_t j = c - reach > 0 ? (c - reach) / l2 : 0; /* (2j + 1) L <= c - 2 D + L: at or left of the first tap */
    if (j > 0) j--;
    while (j < (int64_t)cl && RSZ_M(j) >= reach) j++;
    int64_t nn[RSZ_MAX_TAPS], T = 0, best = 0;
    uint32_t cnt = 0, best_k = 0;
    for (; j < (int64_t)cl && RSZ_M(j) < reach; j++) {
        if (cnt == RSZ_MAX_TAPS) return 0;
        if (cnt == 0) *first = (uint32_t)j;
        nn[cnt] = rsz_cubic_n(RSZ_M(j), D);
        T += nn[cnt];
        if (cnt == 0 || nn[cnt] > best) { best = nn[cnt]; best_k = cnt; }
        cnt++;
    }
#undef RSZ_M
    if (cnt == 0 || cnt > w_cap || T <= 0) return 0;
    int64_t q[RSZ_MAX_TAPS], sum = 0, abs_sum = 0;
    for (uint32_t k = 0; k < cnt; k++) {
        const int64_t num = nn[k] * 16384 + (T >> 1);
        q[k] = num >= 0 ? num / T : -((-num + T - 1) / T); /* floor */
        sum += q[k];
    }
    q[best_k] += 16384 - sum;
    for (uint32_t k = 0; k < cnt; k++) abs_sum += q[k] < 0 ? -q[k] : q[k];
    if (abs_sum > 32768) return 0;
    for (uint32_t k = 0; k < cnt; k++) w[k] = (int16_t)q[k];
    return cnt;
}

/* the axis tables of one call (include/debig_hip.h: layout), one per distinct (cl, L) */
typedef struct rsz_axis { uint32_t cl, max_taps; uint64_t off; } rsz_axis;
typedef struct rsz_tables {
    uint8_t *buf;
    uint64_t len, cap;
    rsz_axis *ax;
    uint32_t n_ax, cap_ax, L, aa, filter;
} rsz_tables;

/* the table of crop length cl (made on first use) -> its index, or -1 (out of memory) */
static int64_t rsz_axis_get(rsz_tables *T, uint32_t cl)
{
    for (uint32_t k = 0; k < T->n_ax; k++)
        if (T->ax[k].cl == cl) return k;
    if (!grow((void **)&T->ax, &T->cap_ax, T->n_ax, sizeof(rsz_axis))) return -1;
    const uint32_t L = T->L;
    int16_t w[RSZ_MAX_TAPS];
    uint32_t first, mt = 1;
    for (uint32_t X = 0; X < L; X++) {
        const uint32_t cnt = debig_png_resize_weights_filter(T->filter, cl, L, T->aa, X, &first, w, RSZ_MAX_TAPS);
        if (cnt > mt) mt = cnt;
    }
    const uint64_t bytes = (8u + 8u * (uint64_t)L + 2u * (uint64_t)L * mt + 7u) & ~(uint64_t)7u;
    if (T->len + bytes > T->cap) {
        uint64_t nc = T->cap ? T->cap : 4096;
        while (nc < T->len + bytes) nc *= 2;
        uint8_t *q = (uint8_t *)realloc(T->buf, nc);
        if (!q) return -1;
        T->buf = q;
        T->cap = nc;
    }
    uint8_t *base = T->buf + T->len;
    memset(base, 0, bytes);
    uint32_t *hdr = (uint32_t *)base;
    int16_t *wt = (int16_t *)(base + 8u + 8u * (uint64_t)L);
    hdr[0] = mt;
    hdr[1] = L;
    for (uint32_t X = 0; X < L; X++) {
        hdr[3 + 2 * X] = debig_png_resize_weights_filter(T->filter, cl, L, T->aa, X, &hdr[2 + 2 * X], wt + (uint64_t)X * mt, mt);
    }
    rsz_axis *a = &T->ax[T->n_ax];
    a->cl = cl;
    a->max_taps = mt;
    a->off = T->len;
    T->len += bytes;
    return T->n_ax++;
}

static int rsz_finite(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

/* the argument checks of debig_png_decode_batch_tensor (n > 0): 0, DEBIG_PNG_BAD_FORMAT or DEBIG_PNG_BAD_ARG */
static int tensor_args_check(const void *d_out, const debig_png_tensor_desc *desc)
{
    if (!desc || !d_out || ((uintptr_t)d_out & 15u)) return DEBIG_PNG_BAD_ARG;
    const uint32_t fmt = desc->out_format;
    if ((fmt & ~0x13u) || (fmt & 15u) > DEBIG_PNG_FMT_GRAY_ALPHA || desc->out_layout > DEBIG_PNG_LAYOUT_CHW) return DEBIG_PNG_BAD_FORMAT;
    if (desc->dtype > DEBIG_PNG_T_BF16 || (desc->resize_flags & ~DEBIG_PNG_RESIZE_ANTIALIAS) || desc->out_w == 0 ||
        desc->out_w > 16384u || desc->out_h == 0 || desc->out_h > 16384u)
        return DEBIG_PNG_BAD_ARG;
    if (desc->dtype != DEBIG_PNG_T_UINT)
        for (int k = 0; k < 4; k++)
            if (!rsz_finite(desc->scale[k]) || !rsz_finite(desc->bias[k])) return DEBIG_PNG_BAD_ARG;
    return 0;
}

#define RSZ_TASK_FIELDS (offsetof(debig_png_resize_task, b) + sizeof(((debig_png_resize_task *)0)->b)) /* without tail padding */
_Static_assert(offsetof(debig_png_resize_alpha_task, mode) == RSZ_TASK_FIELDS &&
                   offsetof(debig_png_resize_alpha_task, b) == offsetof(debig_png_resize_task, b) &&
                   sizeof(debig_png_resize_alpha_task) == 128,
               "debig_png_resize_alpha_task starts with the fields of debig_png_resize_task");
_Static_assert(sizeof(debig_png_resize_cubic_task) == sizeof(debig_png_resize_alpha_task) &&
                   offsetof(debig_png_resize_cubic_task, mode) == offsetof(debig_png_resize_alpha_task, mode) &&
                   offsetof(debig_png_resize_cubic_task, src_channels) == offsetof(debig_png_resize_alpha_task, src_channels) &&
                   offsetof(debig_png_resize_cubic_task, out_channels) == offsetof(debig_png_resize_alpha_task, out_channels) &&
                   offsetof(debig_png_resize_cubic_task, bg) == offsetof(debig_png_resize_alpha_task, bg) &&
                   offsetof(debig_png_resize_cubic_task, b) == offsetof(debig_png_resize_alpha_task, b),
               "debig_png_resize_cubic_task has the layout of debig_png_resize_alpha_task (tensor_core fills both through one)");

/* ---- the staging path of the tensor, label and colour-label calls: IHDR, the crop box and the image's place in the context's
 *      own arena (c->rsz_src), then the decode into it; and the way their tasks and tables reach the device ------------------- */

/* what the three calls' staging differs in */
typedef struct stage_rule {
    uint32_t fmt;          /* the arena's format; GRAY | NATIVE_DEPTH (labels): one element per pixel, as wide as the file's samples */
    uint32_t labels;       /* spec_target.labels */
    uint32_t index_only;   /* != 0: colour types 2, 4 and 6 are E_LABEL */
    uint32_t no16;         /* != 0: a 16-bit file is E_LABEL */
    uint64_t max_w, max_h; /* max_w != 0: a crop wider / taller than this is E_BOX (the antialiased resize) */
    const uint8_t *warp_bad; /* != NULL: file i with warp_bad[i] != 0 is E_WARP (the warp calls) */
    const uint8_t *color_bad; /* != NULL: file i with color_bad[i] != 0 is E_COLOR (the colour-matrix calls) */
    const uint8_t *tone_bad; /* != NULL: file i with tone_bad[i] != 0 is E_TONE (the tone call) */
    const uint8_t *blur_bad; /* != NULL: file i with blur_bad[i] != 0 is E_BLUR (the blur call) */
} stage_rule;

/* per file: the status decided from IHDR (0: none), the image's place and size in the arena, the resolved box, the walk's info */
typedef struct stage {
    uint32_t *pre;
    uint64_t *offs, *caps;
    debig_png_box *box;
    debig_png_info *inf;
} stage;

static void stage_free(stage *S)
{
    free(S->pre);
    free(S->offs);
    free(S->caps);
    free(S->box);
    free(S->inf);
}

/* IHDR -> E_LABEL, then E_BOX, then E_WARP, then E_COLOR, then E_TONE, then E_BLUR, then the walk's own error, then the size cap; the decode of what is left into the arena.
 * -> 0 (status and infos written; S filled, the caller's to stage_free either way) or the call's return value */
static int stage_decode(stage *S, const stage_rule *R, const uint8_t *const *inputs, const uint64_t *input_sizes,
                        const debig_png_box *boxes, uint32_t *status, debig_png_info *infos, uint32_t n, uint32_t flags)
{
    S->pre = (uint32_t *)calloc(n, sizeof(uint32_t));
    S->offs = (uint64_t *)calloc(n, sizeof(uint64_t));
    S->caps = (uint64_t *)calloc(n, sizeof(uint64_t));
    S->box = (debig_png_box *)calloc(n, sizeof(debig_png_box));
    S->inf = (debig_png_info *)calloc(n, sizeof(debig_png_info));
    if (!S->pre || !S->offs || !S->caps || !S->box || !S->inf) return 2;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        spec_file f0;
        memset(&f0, 0, sizeof f0);
        const uint32_t st = spec_walk(inputs[i], input_sizes[i], &f0, 1);
        spec_free(&f0);
        S->offs[i] = total;
        const uint64_t iw = f0.info.width, ih = f0.info.height;
        if (iw == 0) continue; /* no valid IHDR: the walk's status stands */
        const uint32_t ct = f0.info.color_type;
        if ((R->index_only && ct != 0 && ct != 3) || (R->no16 && f0.info.bit_depth == 16)) {
            S->pre[i] = DEBIG_PNG_E_LABEL;
            continue;
        }
        debig_png_box b = {0, 0, (uint32_t)iw, (uint32_t)ih};
        if (boxes && (boxes[i].w || boxes[i].h)) b = boxes[i];
        if (b.w == 0 || b.h == 0 || (uint64_t)b.x + b.w > iw || (uint64_t)b.y + b.h > ih ||
            (R->max_w && (b.w > R->max_w || b.h > R->max_h))) {
            S->pre[i] = DEBIG_PNG_E_BOX;
            continue;
        }
        if (R->warp_bad && R->warp_bad[i]) {
            S->pre[i] = DEBIG_PNG_E_WARP;
            continue;
        }
        if (R->color_bad && R->color_bad[i]) {
            S->pre[i] = DEBIG_PNG_E_COLOR;
            continue;
        }
        if (R->tone_bad && R->tone_bad[i]) {
            S->pre[i] = DEBIG_PNG_E_TONE;
            continue;
        }
        if (R->blur_bad && R->blur_bad[i]) {
            S->pre[i] = DEBIG_PNG_E_BLUR;
            continue;
        }
        S->box[i] = b;
        if (st != DEBIG_PNG_OK) continue;
        const uint64_t sz = fmt_size(iw, ih, fmt_resolve(&f0.info, R->fmt));
        if (sz > RSZ_MAX_IMAGE_BYTES) continue; /* caps[i] stays 0: E_OUTPUT */
        S->caps[i] = sz;
        total += debig_align16(sz) + 16;
    }
    const spec_target tg = {NULL, NULL, S->offs, total + 64, S->pre, R->labels};
    const int rc = spec_decode_core(inputs, input_sizes, &tg, S->caps, status, S->inf, n, flags, R->fmt, DEBIG_PNG_LAYOUT_HWC);
    if (rc == 0 && infos) memcpy(infos, S->inf, (size_t)n * sizeof(debig_png_info));
    return rc;
}

/* a host table of one launch and where it lands in c->rsz_weights; src NULL: the space only, nothing copied */
typedef struct dev_table { const void *src; uint64_t bytes, off; } dev_table;

/* the tables one behind the other, in their order: every off.  Tasks are built with these offsets, after it. */
static void dev_tables_place(dev_table *tab, uint32_t n_tab)
{
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_tab; k++) {
        tab[k].off = at;
        at += tab[k].bytes;
    }
}

/* n_tasks tasks of elem bytes -> c->rsz_tasks, the placed tables -> c->rsz_weights.  -> the context (the launch, which follows
 * on the same stream, takes its pointers from it), or NULL and *rc */
static debig_ctx *dev_upload(const void *tasks, uint64_t n_tasks, size_t elem, const dev_table *tab, uint32_t n_tab, int *rc)
{
    debig_ctx *c = debig_ctx_get(0);
    *rc = 1;
    if (!c) return NULL;
    if ((*rc = debig_devbuf_reserve(&c->rsz_tasks, n_tasks * elem)) ||
        (*rc = debig_devbuf_reserve(&c->rsz_weights, tab[n_tab - 1].off + tab[n_tab - 1].bytes)) ||
        (*rc = debig_hip_memcpy_h2d(c->rsz_tasks.ptr, tasks, n_tasks * elem, NULL)))
        return NULL;
    for (uint32_t k = 0; k < n_tab; k++)
        if (tab[k].src && tab[k].bytes &&
            (*rc = debig_hip_memcpy_h2d((uint8_t *)c->rsz_weights.ptr + tab[k].off, tab[k].src, tab[k].bytes, NULL)))
            return NULL;
    return c;
}

/* the row-run cut: a task is a run of whole rows of at most max_elems elements, or one row when a row is wider.  -> the rows of a
 * full run; run_rows: those of the run that starts in row y0 of h */
static uint32_t row_run(uint32_t w, uint32_t max_elems) { return w >= max_elems ? 1u : max_elems / w; }
static uint32_t run_rows(uint32_t h, uint32_t y0, uint32_t run) { return h - y0 < run ? h - y0 : run; }

/* ---- the per-image colour matrix of the tensor decodes (decode_png.h) --------------------------------------------------------- */

_Static_assert(offsetof(debig_png_resize_color_task, reserved2) == RSZ_TASK_FIELDS && sizeof(debig_png_resize_color_task) == 120 &&
                   offsetof(debig_png_resize_color_task, b) == offsetof(debig_png_resize_task, b) && sizeof(debig_png_color_rec) == 64,
               "debig_png_resize_color_task starts with the fields of debig_png_resize_task");

/* llround of a finite x below 2^62 in magnitude: x - trunc(x) is exact; halves go away from zero */
static int64_t color_llround(double x)
{
    int64_t q = (int64_t)x;
    const double d = x - (double)q;
    if (d >= 0.5) q++;
    else if (d <= -0.5) q--;
    return q;
}

DEBIG_API int debig_png_color_quantise(const double M[12], uint32_t bits, int32_t k[9], int64_t o[3])
{
    if (bits != 8u && bits != 16u) return 0;
    for (uint32_t j = 0; j < 12; j++) {
        uint64_t u;
        memcpy(&u, &M[j], 8);
        if ((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return 0; /* infinity or NaN */
        if ((M[j] < 0 ? -M[j] : M[j]) > 16.0) return 0;
    }
    const double vmax = (double)(((1u << bits) - 1u) << (30u - bits));
    for (uint32_t c = 0; c < 3; c++) {
        for (uint32_t j = 0; j < 3; j++) k[3 * c + j] = (int32_t)color_llround(M[4 * c + j] * 65536.0); /* (exact product) */
        o[c] = color_llround(M[4 * c + 3] * vmax); /* (the product as float64 rounds it, below 2^34) */
    }
    return 1;
}

/* the files' matrices as device records and their E_COLOR flags; -> 0 or 2 */
static int color_prepare(const debig_png_color *colors, uint32_t n, uint32_t bits, debig_png_color_rec **rec, uint8_t **bad)
{
    *rec = (debig_png_color_rec *)calloc(n, sizeof(debig_png_color_rec));
    *bad = (uint8_t *)calloc(n, 1);
    if (!*rec || !*bad) return 2;
    for (uint32_t i = 0; i < n; i++) (*bad)[i] = !debig_png_color_quantise(colors[i].m, bits, (*rec)[i].k, (*rec)[i].o);
    return 0;
}

/* ---- the tone curves of the tensor decode (decode_png.h: debig_png_decode_batch_tensor_tone) -------------------------------- */

_Static_assert(sizeof(debig_png_tone_task) == 96, "debig_png_tone_task: 96 bytes, no padding");

/* the E_TONE rule of one file */
static int tone_param_ok(uint32_t op, uint32_t param, uint32_t n_tables)
{
    switch (op) {
    case DEBIG_PNG_TONE_NONE:
    case DEBIG_PNG_TONE_AUTOCONTRAST:
    case DEBIG_PNG_TONE_EQUALIZE: return param == 0;
    case DEBIG_PNG_TONE_POSTERIZE: return param >= 1 && param <= 8;
    case DEBIG_PNG_TONE_SOLARIZE: return param <= 256;
    case DEBIG_PNG_TONE_TABLE: return param < n_tables;
    default: return 0;
    }
}

DEBIG_API int debig_png_tone_table(uint32_t op, uint32_t param, const uint32_t hist[256], uint8_t lut[256])
{
    if (op == DEBIG_PNG_TONE_NONE || op == DEBIG_PNG_TONE_TABLE || !tone_param_ok(op, param, 0)) return 0;
    if (op == DEBIG_PNG_TONE_POSTERIZE) {
        for (uint32_t i = 0; i < 256; i++) lut[i] = (uint8_t)(i & ~((1u << (8u - param)) - 1u));
        return 1;
    }
    if (op == DEBIG_PNG_TONE_SOLARIZE) {
        for (uint32_t i = 0; i < 256; i++) lut[i] = (uint8_t)(i < param ? i : 255u - i);
        return 1;
    }
    if (!hist) return 0;
    uint32_t lo = 0, hi = 0, nz = 0;
    uint64_t total = 0; /* (the device's counts fit 32 bits; any 256 uint32 fit 40) */
    for (uint32_t i = 0; i < 256; i++) {
        if (!hist[i]) continue;
        if (!nz++) lo = i;
        hi = i;
        total += hist[i];
    }
    for (uint32_t i = 0; i < 256; i++) lut[i] = (uint8_t)i;
    if (nz < 2) return 1;
    if (op == DEBIG_PNG_TONE_AUTOCONTRAST) {
        for (uint32_t i = 0; i < 256; i++) {
            const uint32_t v = i < lo ? 0 : (i - lo) * 255u / (hi - lo);
            lut[i] = (uint8_t)(v < 255u ? v : 255u);
        }
        return 1;
    }
    const uint64_t step = (total - hist[hi]) / 255u;
    if (step == 0) return 1;
    uint64_t acc = step / 2u;
    for (uint32_t i = 0; i < 256; i++) {
        const uint64_t v = acc / step;
        lut[i] = (uint8_t)(v < 255u ? v : 255u);
        acc += hist[i];
    }
    return 1;
}

/* ---- Gaussian blur and sharpness of the tensor decode (decode_png.h: debig_png_decode_batch_tensor_blur) ---------------------- */

_Static_assert(sizeof(debig_png_blur_task) == 104, "debig_png_blur_task: 104 bytes, no padding");

/* the E_BLUR rule of one file */
static int blur_param_ok(const debig_png_blur *b)
{
    uint64_t u;
    memcpy(&u, &b->value, 8);
    const int finite = (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; /* neither infinity nor NaN */
    switch (b->op) {
    case DEBIG_PNG_BLUR_NONE: return 1;
    case DEBIG_PNG_BLUR_GAUSSIAN:
        return (b->ksize & 1u) && b->ksize >= 3u && b->ksize <= 63u && finite && b->value > 0.0 && b->value <= 1000.0;
    case DEBIG_PNG_BLUR_SHARPNESS: return finite && b->value >= -16.0 && b->value <= 16.0;
    default: return 0;
    }
}

DEBIG_API int debig_png_blur_weights(uint32_t ksize, double sigma, int16_t q[63])
{
    const debig_png_blur b = {DEBIG_PNG_BLUR_GAUSSIAN, ksize, sigma};
    if (!blur_param_ok(&b)) return 0;
    const int32_t r = (int32_t)(ksize / 2u);
    double w[63], sum = 0.0;
    for (int32_t j = -r; j <= r; j++) {
        const double t = (double)j / sigma;
        sum += w[j + r] = exp(-0.5 * (t * t));
    }
    int32_t total = 0;
    memset(q, 0, 63 * sizeof(int16_t));
    for (uint32_t j = 0; j < ksize; j++) {
        q[j] = (int16_t)(w[j] / sum * 16384.0 + 0.5); /* (non-negative: the cast is the floor) */
        total += q[j];
    }
    q[r] = (int16_t)(q[r] + (16384 - total)); /* (the deficit is below 32 in magnitude, the centre weight is at least 16384 / 63) */
    return 1;
}

/* what the tone and blur calls add to a tensor core: per file its E_TONE and E_BLUR flags and, once the statuses are known, the
 * place of a decoded file that has a tone or a blur operation among the 8-bit intermediates (UINT32_MAX: none), and the place
 * of a file that has both among the second intermediates, which lie behind the first in the same arena */
#define POST_TONE_REC 256u /* a file's bytes among the uploaded tables: its tone table ...                                    */
#define POST_BLUR_REC 384u /* ... and, in the blur call, its 63 int16 weights and a zero behind it                            */
typedef struct tone_plan {
    const debig_png_tone *tones; /* NULL (the blur call only): no file has a tone operation */
    const uint8_t *tables;
    uint32_t n_tables;
    const debig_png_blur *blurs; /* NULL: the tone call */
    uint32_t oc;         /* the channels of the tensor */
    uint8_t *bad, *blur_bad;
    uint32_t *place, *place2;
    uint8_t *lut;        /* 16 bytes of slack, then rec bytes per placed file */
    uint32_t rec;
    debig_png_tone_task *tasks;
    debig_png_blur_task *btasks;
    uint32_t n_tone, n_both;
    uint64_t img;        /* bytes of one intermediate, a multiple of 16 */
} tone_plan;

static void tone_free(tone_plan *tp)
{
    if (!tp) return;
    free(tp->bad);
    free(tp->blur_bad);
    free(tp->place);
    free(tp->place2);
    free(tp->lut);
    free(tp->tasks);
    free(tp->btasks);
}

static uint32_t tone_op(const tone_plan *tp, uint32_t i) { return tp->tones ? tp->tones[i].op : DEBIG_PNG_TONE_NONE; }
static uint32_t blur_op(const tone_plan *tp, uint32_t i) { return tp->blurs ? tp->blurs[i].op : DEBIG_PNG_BLUR_NONE; }

/* the E_TONE and E_BLUR flags; -> 0 or 2 */
static int tone_prepare(tone_plan *tp, uint32_t n)
{
    if (!tp) return 0;
    tp->bad = (uint8_t *)calloc(n, 1);
    tp->blur_bad = tp->blurs ? (uint8_t *)calloc(n, 1) : NULL;
    tp->place = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
    tp->place2 = (uint32_t *)malloc((size_t)n * sizeof(uint32_t));
    if (!tp->bad || !tp->place || !tp->place2 || (tp->blurs && !tp->blur_bad)) return 2;
    for (uint32_t i = 0; i < n; i++) {
        if (tp->tones) tp->bad[i] = !tone_param_ok(tp->tones[i].op, tp->tones[i].param, tp->n_tables);
        if (tp->blurs) tp->blur_bad[i] = !blur_param_ok(&tp->blurs[i]);
        tp->place[i] = tp->place2[i] = UINT32_MAX;
    }
    return 0;
}

/* after the decode: the places of the files with an operation, and room for their tables; -> 0 or 2 */
static int tone_place(tone_plan *tp, const uint32_t *status, uint32_t n, uint32_t W, uint32_t H)
{
    if (!tp) return 0;
    tp->img = debig_align16((uint64_t)W * H * tp->oc);
    tp->rec = tp->blurs ? POST_BLUR_REC : POST_TONE_REC;
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] != DEBIG_PNG_OK) continue;
        const int t = tone_op(tp, i) != DEBIG_PNG_TONE_NONE, b = blur_op(tp, i) != DEBIG_PNG_BLUR_NONE;
        if (t || b) tp->place[i] = tp->n_tone++;
        if (t && b) tp->place2[i] = tp->n_both++;
    }
    tp->lut = (uint8_t *)calloc((size_t)tp->n_tone * tp->rec + 16u, 1);
    return tp->lut ? 0 : 2;
}

static int tone_is(const tone_plan *tp, uint32_t i) { return tp && tp->place[i] != UINT32_MAX; }
static uint64_t tone_table_bytes(const tone_plan *tp) { return tp ? (uint64_t)tp->n_tone * tp->rec + 16u : 0; }
static uint64_t tone_arena_bytes(const tone_plan *tp) { return ((uint64_t)tp->n_tone + tp->n_both) * tp->img; }

/* the tables at their place: the table lands at table_off in the weights buffer, its first record at the next multiple of
 * 16 -> that offset */
static uint64_t tone_fill(tone_plan *tp, uint32_t n, uint64_t table_off)
{
    const uint64_t pad = (16u - (table_off & 15u)) & 15u;
    for (uint32_t i = 0; i < n; i++) {
        if (tp->place[i] == UINT32_MAX) continue;
        uint8_t *l = tp->lut + pad + (size_t)tp->place[i] * tp->rec;
        if (tp->tones) {
            const debig_png_tone o = tp->tones[i];
            if (o.op == DEBIG_PNG_TONE_TABLE) memcpy(l, tp->tables + (size_t)o.param * 256u, 256);
            else if (o.op == DEBIG_PNG_TONE_POSTERIZE || o.op == DEBIG_PNG_TONE_SOLARIZE) (void)debig_png_tone_table(o.op, o.param, NULL, l);
        }
        if (blur_op(tp, i) == DEBIG_PNG_BLUR_GAUSSIAN) {
            int16_t q[64] = {0};
            (void)debig_png_blur_weights(tp->blurs[i].ksize, tp->blurs[i].value, q);
            memcpy(l + POST_TONE_REC, q, sizeof q);
        }
    }
    return table_off + pad;
}

/* the first stage has been launched: the pixel runs of every file with a tone operation -- first those whose result is the
 * caller's, then those that a blur follows, which write UINT8 HWC into the second intermediates; in either group those with a
 * histogram first --, the cleared histograms, the histogram kernel over the front of either group and the apply kernel over
 * either group, on the same stream.  lut_off: where tone_fill put the tables in c->rsz_weights.  -> 0 or the call's return value */
static int tone_run(tone_plan *tp, debig_ctx *c, void *d_out, uint32_t n, const debig_png_tensor_desc *desc, uint64_t lut_off)
{
    if (!tp || !tp->tones || tp->n_tone == 0) return 0;
    const uint32_t W = desc->out_w, H = desc->out_h, oc = tp->oc, cc = oc & 1u ? oc : oc - 1u, px = W * H;
    const uint32_t es = desc->dtype == DEBIG_PNG_T_UINT ? 1u : desc->dtype == DEBIG_PNG_T_F32 ? 4u : 2u;
    const uint64_t slot = (uint64_t)px * oc * es;
    uint64_t n_files = 0;
    for (uint32_t i = 0; i < n; i++) n_files += tp->place[i] != UINT32_MAX && tone_op(tp, i) != DEBIG_PNG_TONE_NONE;
    const uint64_t per = (px + DEBIG_PNG_TONE_RUN - 1u) / DEBIG_PNG_TONE_RUN, n_tasks = per * n_files;
    if (n_tasks == 0) return 0;
    if (n_tasks > 0x7fffffffu) return 2;
    tp->tasks = (debig_png_tone_task *)calloc((size_t)n_tasks, sizeof(debig_png_tone_task));
    if (!tp->tasks) return 2;
    uint64_t at = 0, first[2] = {0, 0}, cnt[2] = {0, 0}, n_hist_tasks[2] = {0, 0};
    uint32_t n_hist = 0;
    for (uint32_t part = 0; part < 2; part++) {
        first[part] = at;
        for (uint32_t pass = 0; pass < 2; pass++) {
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t op = tone_op(tp, i);
                if (tp->place[i] == UINT32_MAX || op == DEBIG_PNG_TONE_NONE || (tp->place2[i] != UINT32_MAX) != part) continue;
                const uint32_t hist = op == DEBIG_PNG_TONE_AUTOCONTRAST || op == DEBIG_PNG_TONE_EQUALIZE;
                if (hist == pass) continue;
                const int chw = !part && desc->out_layout == DEBIG_PNG_LAYOUT_CHW;
                debig_png_tone_task p;
                memset(&p, 0, sizeof p);
                p.src_off = (uint64_t)tp->place[i] * tp->img;
                p.out_off = part ? ((uint64_t)tp->n_tone + tp->place2[i]) * tp->img : (uint64_t)i * slot;
                p.hist_off = hist ? (uint64_t)n_hist++ * cc * 1024u : 0;
                p.lut_off = lut_off + (uint64_t)tp->place[i] * tp->rec;
                p.out_w = W;
                p.out_h = H;
                p.out_sx = chw ? 1u : oc;
                p.out_sy = chw ? W : W * oc;
                p.out_sc = chw ? H * W : 1u;
                p.channels = (uint8_t)oc;
                p.colour_channels = (uint8_t)cc;
                p.dtype = (uint8_t)(part ? DEBIG_PNG_T_UINT : desc->dtype);
                p.op = (uint8_t)op;
                for (uint32_t k = 0; k < 4; k++) {
                    p.a[k] = (float)((double)desc->scale[k] / (255.0 * (double)(1u << 22)));
                    p.b[k] = desc->bias[k];
                }
                for (uint32_t p0 = 0; p0 < px; p0 += DEBIG_PNG_TONE_RUN) {
                    p.pix0 = p0;
                    p.pix_n = px - p0 < DEBIG_PNG_TONE_RUN ? px - p0 : DEBIG_PNG_TONE_RUN;
                    tp->tasks[at++] = p;
                }
            }
            if (pass == 0) n_hist_tasks[part] = at - first[part];
        }
        cnt[part] = at - first[part];
    }
    int rc;
    if ((rc = debig_devbuf_reserve(&c->tone_tasks, n_tasks * sizeof(debig_png_tone_task))) ||
        (rc = debig_devbuf_reserve(&c->tone_hist, (uint64_t)n_hist * cc * 1024u + 16u)) ||
        (rc = debig_hip_memcpy_h2d(c->tone_tasks.ptr, tp->tasks, n_tasks * sizeof(debig_png_tone_task), NULL)) ||
        (n_hist && (rc = debig_hip_memset(c->tone_hist.ptr, 0, (uint64_t)n_hist * cc * 1024u, NULL))))
        return rc;
    const debig_png_tone_task *d_tasks = (const debig_png_tone_task *)c->tone_tasks.ptr;
    for (uint32_t part = 0; part < 2; part++)
        if (n_hist_tasks[part] &&
            (rc = debig_hip_png_tone_hist_batch(c->tone_px.ptr, (uint32_t *)c->tone_hist.ptr, d_tasks + first[part],
                                                (uint32_t)n_hist_tasks[part], NULL)))
            return rc;
    for (uint32_t part = 0; part < 2; part++) /* (the tone call has no second part: its launches are what they were) */
        if (cnt[part] &&
            (rc = debig_hip_png_tone_apply_batch(c->tone_px.ptr, part ? c->tone_px.ptr : d_out, d_tasks + first[part],
                                                 (const uint32_t *)c->tone_hist.ptr, c->rsz_weights.ptr, (uint32_t)cnt[part], NULL)))
            return rc;
    return 0;
}

/* behind tone_run: the tiles of every file with a blur operation, from its first intermediate or, where a tone operation came
 * in between, from its second, through the blur kernel into the caller's tensor, on the same stream.  -> 0 or the call's return
 * value */
static int blur_run(tone_plan *tp, debig_ctx *c, void *d_out, uint32_t n, const debig_png_tensor_desc *desc, uint64_t lut_off)
{
    if (!tp || !tp->blurs || tp->n_tone == 0) return 0;
    const uint32_t W = desc->out_w, H = desc->out_h, oc = tp->oc, cc = oc & 1u ? oc : oc - 1u;
    const uint32_t es = desc->dtype == DEBIG_PNG_T_UINT ? 1u : desc->dtype == DEBIG_PNG_T_F32 ? 4u : 2u;
    const uint64_t slot = (uint64_t)W * H * oc * es;
    uint64_t n_tasks = 0, at = 0;
    for (uint32_t fill = 0; fill < 2; fill++) { /* count, then write */
        if (fill) {
            if (n_tasks == 0) return 0;
            if (n_tasks > 0x7fffffffu) return 2;
            tp->btasks = (debig_png_blur_task *)calloc((size_t)n_tasks, sizeof(debig_png_blur_task));
            if (!tp->btasks) return 2;
        }
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t op = blur_op(tp, i);
            if (tp->place[i] == UINT32_MAX || op == DEBIG_PNG_BLUR_NONE) continue;
            const uint32_t r = op == DEBIG_PNG_BLUR_GAUSSIAN ? tp->blurs[i].ksize / 2u : 1u;
            const uint32_t tw = DEBIG_PNG_BLUR_TILE, th = DEBIG_PNG_BLUR_TILE; /* (fits the two LDS caps at every radius) */
            if (!fill) {
                n_tasks += (uint64_t)((W + tw - 1u) / tw) * ((H + th - 1u) / th);
                continue;
            }
            const int chw = desc->out_layout == DEBIG_PNG_LAYOUT_CHW;
            debig_png_blur_task p;
            memset(&p, 0, sizeof p);
            p.src_off = (tp->place2[i] != UINT32_MAX ? (uint64_t)tp->n_tone + tp->place2[i] : (uint64_t)tp->place[i]) * tp->img;
            p.out_off = (uint64_t)i * slot;
            p.table_off = lut_off + (uint64_t)tp->place[i] * tp->rec + POST_TONE_REC;
            p.k = op == DEBIG_PNG_BLUR_SHARPNESS ? (int32_t)color_llround(tp->blurs[i].value * 65536.0) : 0; /* (exact product) */
            p.radius = r;
            p.w = W;
            p.h = H;
            p.out_sx = chw ? 1u : oc;
            p.out_sy = chw ? W : W * oc;
            p.out_sc = chw ? H * W : 1u;
            p.channels = (uint8_t)oc;
            p.colour_channels = (uint8_t)cc;
            p.dtype = (uint8_t)desc->dtype;
            p.op = (uint8_t)op;
            for (uint32_t k = 0; k < 4; k++) {
                p.a[k] = (float)((double)desc->scale[k] / (255.0 * (double)(1u << 22)));
                p.b[k] = desc->bias[k];
            }
            for (uint32_t y0 = 0; y0 < H; y0 += th) {
                for (uint32_t x0 = 0; x0 < W; x0 += tw) {
                    p.x0 = x0;
                    p.y0 = y0;
                    p.tile_w = W - x0 < tw ? W - x0 : tw;
                    p.tile_h = H - y0 < th ? H - y0 : th;
                    tp->btasks[at++] = p;
                }
            }
        }
    }
    int rc;
    if ((rc = debig_devbuf_reserve(&c->blur_tasks, n_tasks * sizeof(debig_png_blur_task))) ||
        (rc = debig_hip_memcpy_h2d(c->blur_tasks.ptr, tp->btasks, n_tasks * sizeof(debig_png_blur_task), NULL)))
        return rc;
    return debig_hip_png_blur_batch(c->tone_px.ptr, d_out, (const debig_png_blur_task *)c->blur_tasks.ptr, c->rsz_weights.ptr,
                                    (uint32_t)n_tasks, NULL);
}

/* debig_png_decode_batch_tensor (amode == DEBIG_PNG_ALPHA_STRAIGHT: bg unused), debig_png_decode_batch_tensor_alpha and
 * debig_png_decode_batch_tensor_filter behind their argument checks.  With alpha the pixels are decoded WITH their alpha (dfmt:
 * 4 or 2 channels) and the tiles go to the alpha kernel, which writes the channels of desc->out_format.  The filter picks the
 * weight rule and the E_BOX scale; BICUBIC tiles, of every alpha mode, go to the signed kernel (debig_hip_png_resize_cubic_batch),
 * NEAREST ones to the kernels of BILINEAR.  colors != NULL (debig_png_decode_batch_tensor_color: STRAIGHT, not BICUBIC, 3 or 4
 * channels): the tiles carry the offset of their image's record, which travels as a third table, and go to the colour kernel.
 * tp != NULL (debig_png_decode_batch_tensor_tone, debig_png_decode_batch_tensor_blur): the tiles of a file with a tone or a blur
 * operation are UINT8 HWC tiles into the context's tone arena; they come behind all others, and the kernel is launched once per
 * target over its range of the one task array; tone_run and blur_run do the rest. */
/* one range of the uploaded tiles through the kernel of the call */
static int tensor_launch(const debig_ctx *c, void *out, const uint8_t *d_tasks, uint64_t cnt, int colors, uint32_t filter, int plain)
{
    return colors ? debig_hip_png_resize_color_batch(c->rsz_src.ptr, out, (const debig_png_resize_color_task *)d_tasks,
                                                     c->rsz_weights.ptr, (uint32_t)cnt, NULL)
           : filter == DEBIG_PNG_FILTER_BICUBIC
               ? debig_hip_png_resize_cubic_batch(c->rsz_src.ptr, out, (const debig_png_resize_cubic_task *)d_tasks,
                                                  c->rsz_weights.ptr, (uint32_t)cnt, NULL)
           : plain ? debig_hip_png_resize_batch(c->rsz_src.ptr, out, (const debig_png_resize_task *)d_tasks, c->rsz_weights.ptr,
                                                (uint32_t)cnt, NULL)
                   : debig_hip_png_resize_alpha_batch(c->rsz_src.ptr, out, (const debig_png_resize_alpha_task *)d_tasks,
                                                      c->rsz_weights.ptr, (uint32_t)cnt, NULL);
}

static int tensor_core(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out, const debig_png_box *boxes,
                       uint32_t *status, debig_png_info *infos, uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc,
                       uint32_t amode, const uint16_t *bg, uint32_t filter, const debig_png_color *colors, tone_plan *tp)
{
    /* fmt: the format decoded into the arena (ch channels); oc: the channels of the tensor */
    uint32_t fmt = desc->out_format;
    const uint32_t oc = fmt_channels(fmt);
    if (amode == DEBIG_PNG_ALPHA_OVER)
        fmt = (fmt & ~15u) | ((fmt & 15u) == DEBIG_PNG_FMT_RGB ? DEBIG_PNG_FMT_RGBA : DEBIG_PNG_FMT_GRAY_ALPHA);
    const uint32_t aa = desc->resize_flags & DEBIG_PNG_RESIZE_ANTIALIAS, W = desc->out_w, H = desc->out_h;
    const uint32_t ch = fmt_channels(fmt), bits = fmt & DEBIG_PNG_FMT_16 ? 16u : 8u, sb = bits / 8u;
    const uint32_t es = desc->dtype == DEBIG_PNG_T_UINT ? sb : desc->dtype == DEBIG_PNG_T_F32 ? 4u : 2u;
    const uint64_t slot = (uint64_t)H * W * oc * es;
    /* the plain kernel's task, or the alpha kernel's and the signed kernel's of one layout: the plain one (channels: the
     * source's) + mode, channel counts, background */
    const int plain = amode == DEBIG_PNG_ALPHA_STRAIGHT && filter != DEBIG_PNG_FILTER_BICUBIC;
    const size_t elem = colors ? sizeof(debig_png_resize_color_task) : plain ? sizeof(debig_png_resize_task) : sizeof(debig_png_resize_alpha_task);
    /* the largest antialiased scale (decode_png.h); NEAREST ignores the flag */
    const uint64_t max_scale = filter == DEBIG_PNG_FILTER_BICUBIC ? 32u : 64u;
    const int aa_box = aa && filter != DEBIG_PNG_FILTER_NEAREST;
    stage S = {NULL, NULL, NULL, NULL, NULL};
    uint8_t *tasks = NULL, *cbad = NULL;
    debig_png_color_rec *crec = NULL;
    rsz_tables TX = {NULL, 0, 0, NULL, 0, 0, W, aa, filter}, TY = {NULL, 0, 0, NULL, 0, 0, H, aa, filter};
    int rc;
    if (colors && (rc = color_prepare(colors, n, bits, &crec, &cbad))) goto done;
    if ((rc = tone_prepare(tp, n))) goto done;
    const stage_rule rule = {fmt, 0, 0, 0, aa_box ? max_scale * W : 0, max_scale * H, NULL, cbad, tp ? tp->bad : NULL, tp ? tp->blur_bad : NULL};
    if ((rc = stage_decode(&S, &rule, inputs, input_sizes, boxes, status, infos, n, flags))) goto done;
    if ((rc = tone_place(tp, status, n, W, H))) goto done;
    /* ---- the axis tables of every decoded image, then their places behind one another */
    rc = 2;
    for (uint32_t i = 0; i < n; i++)
        if (status[i] == DEBIG_PNG_OK && (rsz_axis_get(&TX, S.box[i].w) < 0 || rsz_axis_get(&TY, S.box[i].h) < 0)) goto done;
    dev_table tab[4] = {{TX.buf, TX.len, 0}, {TY.buf, TY.len, 0}, {crec, colors ? (uint64_t)n * sizeof *crec : 0, 0},
                        {tp ? tp->lut : NULL, tone_table_bytes(tp), 0}};
    const uint32_t n_tab = tp ? 4u : colors ? 3u : 2u;
    dev_tables_place(tab, n_tab); /* (the axis tables are multiples of 8 bytes long: the records are 8-byte aligned) */
    const uint64_t lut_off = tp ? tone_fill(tp, n, tab[3].off) : 0;
    /* ---- the tiles of every decoded image; with tp those of the tone files last, n_direct tiles in front of them */
    uint64_t n_tasks = 0, n_direct = 0;
    uint32_t cap_tasks = 0;
    for (uint64_t q = 0; q < (tp ? 2u : 1u) * (uint64_t)n; q++) { /* (with tp: every file twice, the tone files the second time) */
        const uint32_t pass = q >= n, i = (uint32_t)(pass ? q - n : q);
        if (q == n) n_direct = n_tasks;
        if (status[i] != DEBIG_PNG_OK || tone_is(tp, i) != (int)pass) continue;
        const rsz_axis *ax = &TX.ax[rsz_axis_get(&TX, S.box[i].w)], *ay = &TY.ax[rsz_axis_get(&TY, S.box[i].h)];
        const uint32_t mtx = ax->max_taps, mty = ay->max_taps;
        const uint32_t *ey = (const uint32_t *)(TY.buf + ay->off) + 2;
        uint32_t tw = W < DEBIG_PNG_RESIZE_TILE_W ? W : DEBIG_PNG_RESIZE_TILE_W;
        if (tw > DEBIG_PNG_RESIZE_WX_CAP / mtx) tw = DEBIG_PNG_RESIZE_WX_CAP / mtx;
        if (tw > DEBIG_PNG_RESIZE_HQ_CAP / (mty * ch)) tw = DEBIG_PNG_RESIZE_HQ_CAP / (mty * ch);
        debig_png_resize_alpha_task proto; /* (the plain task: its first elem bytes) */
        memset(&proto, 0, sizeof proto);
        proto.src_off = S.offs[i] + ((uint64_t)S.box[i].y * S.inf[i].width + S.box[i].x) * ch * sb;
        proto.out_off = (uint64_t)i * slot;
        proto.wx_off = tab[0].off + ax->off;
        proto.wy_off = tab[1].off + ay->off;
        proto.src_pitch = S.inf[i].width * ch;
        proto.out_sx = desc->out_layout == DEBIG_PNG_LAYOUT_CHW ? 1u : oc;
        proto.out_sy = desc->out_layout == DEBIG_PNG_LAYOUT_CHW ? W : W * oc;
        proto.out_sc = desc->out_layout == DEBIG_PNG_LAYOUT_CHW ? H * W : 1u;
        proto.channels = (uint8_t)ch;
        proto.bits = (uint8_t)bits;
        proto.dtype = (uint8_t)desc->dtype;
        for (uint32_t k = 0; k < 4; k++) {
            proto.a[k] = (float)((double)desc->scale[k] / ((double)((1u << bits) - 1u) * (double)(1u << (30u - bits))));
            proto.b[k] = desc->bias[k];
        }
        if (pass) { /* the 8-bit HWC intermediate */
            proto.out_off = (uint64_t)tp->place[i] * tp->img;
            proto.out_sx = oc;
            proto.out_sy = W * oc;
            proto.out_sc = 1u;
            proto.dtype = DEBIG_PNG_T_UINT;
        }
        proto.mode = amode;
        proto.src_channels = (uint8_t)ch;
        proto.out_channels = (uint8_t)oc;
        if (amode == DEBIG_PNG_ALPHA_OVER)
            for (uint32_t j = 0; j < oc; j++) proto.bg[j] = bg[j];
        for (uint32_t y0 = 0; y0 < H;) {
            uint32_t lo = ey[2 * y0], hi = ey[2 * y0] + ey[2 * y0 + 1], th = 1;
            while (y0 + th < H && th < 64u) {
                const uint32_t f = ey[2 * (y0 + th)], e = f + ey[2 * (y0 + th) + 1];
                const uint32_t nlo = f < lo ? f : lo, nhi = e > hi ? e : hi;
                if ((uint64_t)(nhi - nlo) * tw * ch > DEBIG_PNG_RESIZE_HQ_CAP) break;
                lo = nlo;
                hi = nhi;
                th++;
            }
            for (uint32_t x0 = 0; x0 < W; x0 += tw) {
                if (n_tasks >= 0x7fffffffu || !grow((void **)&tasks, &cap_tasks, (uint32_t)n_tasks, elem)) goto done;
                debig_png_resize_task *t = (debig_png_resize_task *)(tasks + n_tasks++ * elem);
                if (colors) { /* the plain task's fields, then the record's place */
                    debig_png_resize_color_task *ct = (debig_png_resize_color_task *)t;
                    memset(ct, 0, sizeof *ct);
                    memcpy(ct, &proto, RSZ_TASK_FIELDS);
                    ct->color_off = tab[2].off + (uint64_t)i * sizeof *crec;
                } else {
                    memcpy(t, &proto, elem);
                }
                t->tile_x = x0;
                t->tile_y = y0;
                t->tile_w = W - x0 < tw ? W - x0 : tw;
                t->tile_h = th;
                t->src_y0 = lo;
                t->src_rows = hi - lo;
            }
            y0 += th;
        }
    }
    if (!tp) n_direct = n_tasks;
    rc = 0;
    if (n_tasks == 0) goto done;
    debig_ctx *c = dev_upload(tasks, n_tasks, elem, tab, n_tab, &rc);
    if (!c) goto done;
    const uint8_t *d_tasks = (const uint8_t *)c->rsz_tasks.ptr;
    if (n_tasks > n_direct && (rc = debig_devbuf_reserve(&c->tone_px, tone_arena_bytes(tp)))) goto done;
    if ((n_direct && (rc = tensor_launch(c, d_out, d_tasks, n_direct, colors != NULL, filter, plain))) ||
        (n_tasks > n_direct &&
         (rc = tensor_launch(c, c->tone_px.ptr, d_tasks + n_direct * elem, n_tasks - n_direct, colors != NULL, filter, plain))) ||
        (rc = tone_run(tp, c, d_out, n, desc, lut_off)) || (rc = blur_run(tp, c, d_out, n, desc, lut_off)))
        goto done;
    rc = debig_hip_stream_sync(NULL);
done:
    stage_free(&S);
    tone_free(tp);
    free(tasks);
    free(crec);
    free(cbad);
    free(TX.buf);
    free(TX.ax);
    free(TY.buf);
    free(TY.ax);
    return rc;
}

DEBIG_API int debig_png_decode_batch_tensor(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                            const debig_png_box *boxes, uint32_t *status, debig_png_info *infos, uint32_t n,
                                            uint32_t flags, const debig_png_tensor_desc *desc)
{
    /* the arguments on their own, before any file is looked at */
    if (n == 0) return 0;
    const int bad = tensor_args_check(d_out, desc);
    if (bad) return bad;
    return tensor_core(inputs, input_sizes, d_out, boxes, status, infos, n, flags, desc, DEBIG_PNG_ALPHA_STRAIGHT, NULL, DEBIG_PNG_FILTER_BILINEAR, NULL, NULL);
}

/* the checks of debig_png_decode_batch_tensor_alpha (n > 0): those of debig_png_decode_batch_tensor first and unchanged, then
 * alpha's; all before any file is looked at -> 0 and *mode, or the call's return value */
static int tensor_alpha_check(const void *d_out, const debig_png_tensor_desc *desc, const debig_png_alpha_desc *alpha, uint32_t *mode)
{
    const int bad = tensor_args_check(d_out, desc);
    if (bad) return bad;
    uint32_t amode = DEBIG_PNG_ALPHA_STRAIGHT;
    if (alpha) {
        const uint32_t lay = desc->out_format & 15u, bits = desc->out_format & DEBIG_PNG_FMT_16 ? 16u : 8u;
        amode = alpha->mode;
        if (amode > DEBIG_PNG_ALPHA_OVER || alpha->reserved != 0) return DEBIG_PNG_BAD_ARG;
        if (amode == DEBIG_PNG_ALPHA_PREMULTIPLIED && lay != DEBIG_PNG_FMT_RGBA && lay != DEBIG_PNG_FMT_GRAY_ALPHA) return DEBIG_PNG_BAD_ARG;
        if (amode == DEBIG_PNG_ALPHA_OVER) {
            if (lay != DEBIG_PNG_FMT_RGB && lay != DEBIG_PNG_FMT_GRAY) return DEBIG_PNG_BAD_ARG;
            for (uint32_t k = 0; k < fmt_channels(desc->out_format); k++)
                if (alpha->background[k] > (1u << bits) - 1u) return DEBIG_PNG_BAD_ARG;
        }
    }
    *mode = amode;
    return 0;
}

DEBIG_API int debig_png_decode_batch_tensor_alpha(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                  const debig_png_box *boxes, uint32_t *status, debig_png_info *infos,
                                                  uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc,
                                                  const debig_png_alpha_desc *alpha)
{
    if (n == 0) return 0;
    uint32_t amode;
    const int bad = tensor_alpha_check(d_out, desc, alpha, &amode);
    if (bad) return bad;
    return tensor_core(inputs, input_sizes, d_out, boxes, status, infos, n, flags, desc, amode, alpha ? alpha->background : NULL,
                       DEBIG_PNG_FILTER_BILINEAR, NULL, NULL);
}

DEBIG_API int debig_png_decode_batch_tensor_filter(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                   const debig_png_box *boxes, uint32_t *status, debig_png_info *infos,
                                                   uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc,
                                                   const debig_png_alpha_desc *alpha, const debig_png_filter_desc *filter)
{
    /* every check of debig_png_decode_batch_tensor_alpha first and unchanged, then the filter's */
    if (n == 0) return 0;
    uint32_t amode;
    const int bad = tensor_alpha_check(d_out, desc, alpha, &amode);
    if (bad) return bad;
    if (filter && (filter->filter > DEBIG_PNG_FILTER_NEAREST || filter->reserved != 0)) return DEBIG_PNG_BAD_ARG;
    return tensor_core(inputs, input_sizes, d_out, boxes, status, infos, n, flags, desc, amode, alpha ? alpha->background : NULL,
                       filter ? filter->filter : DEBIG_PNG_FILTER_BILINEAR, NULL, NULL);
}

/* the colour matrix goes with three colour channels: RGB or RGBA */
static int color_layout_ok(uint32_t out_format)
{
    return (out_format & 15u) == DEBIG_PNG_FMT_RGB || (out_format & 15u) == DEBIG_PNG_FMT_RGBA;
}

DEBIG_API int debig_png_decode_batch_tensor_color(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                  const debig_png_box *boxes, const debig_png_color *colors, uint32_t *status,
                                                  debig_png_info *infos, uint32_t n, uint32_t flags,
                                                  const debig_png_tensor_desc *desc, const debig_png_filter_desc *filter)
{
    /* every check of debig_png_decode_batch_tensor first and unchanged, then the filter's, then the matrix call's own */
    if (n == 0) return 0;
    const int bad = tensor_args_check(d_out, desc);
    if (bad) return bad;
    if (filter && (filter->filter > DEBIG_PNG_FILTER_NEAREST || filter->reserved != 0)) return DEBIG_PNG_BAD_ARG;
    if (!colors || !color_layout_ok(desc->out_format) || (filter && filter->filter == DEBIG_PNG_FILTER_BICUBIC)) return DEBIG_PNG_BAD_ARG;
    return tensor_core(inputs, input_sizes, d_out, boxes, status, infos, n, flags, desc, DEBIG_PNG_ALPHA_STRAIGHT, NULL,
                       filter ? filter->filter : DEBIG_PNG_FILTER_BILINEAR, colors, NULL);
}

/* ---- debig_png_decode_batch_labels: palette indices / raw grey samples -> one dense integer class-map tensor (decode_png.h) - */

#define LBL_TASK_ELEMS 16384u /* output elements of one gather task (a run of whole rows; one row when it is wider) */

/* the index table of one axis (crop length cl -> L outputs: ((2X + 1) cl) div 2L, 64-bit on the host) appended to *buf,
 * 16-byte aligned; one table per distinct cl.  -> its offset, or UINT64_MAX (out of memory) */
typedef struct lbl_axis { uint32_t cl; uint64_t off; } lbl_axis;
typedef struct lbl_tables { uint32_t *buf; uint64_t len, cap; /* in uint32 */ lbl_axis *ax; uint32_t n_ax, cap_ax, L; } lbl_tables;
static uint64_t lbl_axis_get(lbl_tables *T, uint32_t cl)
{
    for (uint32_t k = 0; k < T->n_ax; k++)
        if (T->ax[k].cl == cl) return T->ax[k].off;
    if (!grow((void **)&T->ax, &T->cap_ax, T->n_ax, sizeof(lbl_axis))) return UINT64_MAX;
    const uint64_t words = ((uint64_t)T->L + 3u) & ~(uint64_t)3u;
    if (T->len + words > T->cap) {
        uint64_t nc = T->cap ? T->cap : 1024;
        while (nc < T->len + words) nc *= 2;
        uint32_t *q = (uint32_t *)realloc(T->buf, nc * sizeof(uint32_t));
        if (!q) return UINT64_MAX;
        T->buf = q;
        T->cap = nc;
    }
    uint32_t *t = T->buf + T->len;
    for (uint64_t X = 0; X < words; X++) t[X] = X < T->L ? (uint32_t)(((2u * X + 1u) * cl) / (2u * (uint64_t)T->L)) : 0u;
    T->ax[T->n_ax].cl = cl;
    T->ax[T->n_ax].off = T->len * sizeof(uint32_t);
    T->n_ax++;
    T->len += words;
    return T->ax[T->n_ax - 1].off;
}

/* the row-run tasks of the label and the colour-label call: both kernels' tasks (elem bytes) start with src_off, out_off,
 * sx_off, sy_off and hold row0 and rows side by side (at row_at) */
typedef struct lbl_head { uint64_t src_off, out_off, sx_off, sy_off; } lbl_head;
_Static_assert(offsetof(debig_png_label_task, sy_off) == offsetof(lbl_head, sy_off) &&
                   offsetof(debig_png_color_label_task, sy_off) == offsetof(lbl_head, sy_off) &&
                   offsetof(debig_png_label_task, rows) == offsetof(debig_png_label_task, row0) + 4 &&
                   offsetof(debig_png_color_label_task, rows) == offsetof(debig_png_color_label_task, row0) + 4,
               "the fields lbl_runs fills lie alike in both label tasks");
typedef struct lbl_job {
    uint8_t *tasks;
    uint64_t n_tasks;
    uint32_t cap_tasks, W, H;
    size_t elem, row_at;
    lbl_tables TX, TY;
    dev_table *tx, *ty; /* their places among the call's tables */
} lbl_job;

/* the axis tables of every decoded image -> *tx, *ty (not placed yet).  -> 0 or 2 */
static int lbl_axes(lbl_job *J, const stage *S, const uint32_t *status, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++)
        if (status[i] == DEBIG_PNG_OK &&
            (lbl_axis_get(&J->TX, S->box[i].w) == UINT64_MAX || lbl_axis_get(&J->TY, S->box[i].h) == UINT64_MAX))
            return 2;
    J->tx->src = J->TX.buf;
    J->tx->bytes = J->TX.len * sizeof(uint32_t);
    J->ty->src = J->TY.buf;
    J->ty->bytes = J->TY.len * sizeof(uint32_t);
    return 0;
}

/* the row runs of one decoded image (px bytes per pixel in the arena): copies of *proto, the caller's task with everything but
 * the fields named above filled in.  -> 0 or 2 */
static int lbl_runs(lbl_job *J, const stage *S, uint32_t i, uint32_t px, uint64_t slot, void *proto)
{
    const uint32_t run = row_run(J->W, LBL_TASK_ELEMS);
    const lbl_head h = {S->offs[i] + ((uint64_t)S->box[i].y * S->inf[i].width + S->box[i].x) * px, (uint64_t)i * slot,
                        J->tx->off + lbl_axis_get(&J->TX, S->box[i].w), J->ty->off + lbl_axis_get(&J->TY, S->box[i].h)};
    memcpy(proto, &h, sizeof h);
    for (uint32_t y0 = 0; y0 < J->H; y0 += run) {
        if (J->n_tasks >= 0x7fffffffu || !grow((void **)&J->tasks, &J->cap_tasks, (uint32_t)J->n_tasks, J->elem)) return 2;
        uint8_t *t = J->tasks + J->n_tasks++ * J->elem;
        const uint32_t rows[2] = {y0, run_rows(J->H, y0, run)};
        memcpy(t, proto, J->elem);
        memcpy(t + J->row_at, rows, sizeof rows);
    }
    return 0;
}

static void lbl_job_free(lbl_job *J)
{
    free(J->tasks);
    free(J->TX.buf);
    free(J->TX.ax);
    free(J->TY.buf);
    free(J->TY.ax);
}

/* the argument checks of debig_png_decode_batch_labels (n > 0): 0 or DEBIG_PNG_BAD_ARG */
static int label_args_check(const void *d_out, const debig_png_label_desc *desc)
{
    if (!desc || !d_out || ((uintptr_t)d_out & 15u)) return DEBIG_PNG_BAD_ARG;
    if (desc->out_w == 0 || desc->out_w > 16384u || desc->out_h == 0 || desc->out_h > 16384u || desc->dtype > DEBIG_PNG_L_I64 ||
        desc->reserved != 0)
        return DEBIG_PNG_BAD_ARG;
    if (desc->lut && desc->dtype <= DEBIG_PNG_L_U16)
        for (uint32_t k = 0; k < 256; k++)
            if (desc->lut[k] < 0 || desc->lut[k] > (desc->dtype == DEBIG_PNG_L_U8 ? 255 : 65535)) return DEBIG_PNG_BAD_ARG;
    return 0;
}

DEBIG_API int debig_png_decode_batch_labels(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                            const debig_png_box *boxes, uint32_t *status, debig_png_info *infos, uint32_t n,
                                            uint32_t flags, const debig_png_label_desc *desc)
{
    /* the arguments on their own, before any file is looked at */
    if (n == 0) return 0;
    const int bad = label_args_check(d_out, desc);
    if (bad) return bad;
    const uint32_t W = desc->out_w, H = desc->out_h, es = 1u << desc->dtype;
    /* E_LABEL: colour type 2, 4 or 6; a 16-bit file with dtype U8 or with a lut */
    const stage_rule rule = {DEBIG_PNG_FMT_GRAY | DEBIG_PNG_FMT_NATIVE_DEPTH, 1, 1, desc->dtype == DEBIG_PNG_L_U8 || desc->lut, 0, 0, NULL, NULL, NULL, NULL};

    stage S = {NULL, NULL, NULL, NULL, NULL};
    dev_table tab[3] = {{desc->lut, 1024, 0}, {NULL, 0, 0}, {NULL, 0, 0}}; /* the LUT (or its room), the X tables, the Y tables */
    lbl_job J = {NULL, 0, 0, W, H, sizeof(debig_png_label_task), offsetof(debig_png_label_task, row0),
                 {NULL, 0, 0, NULL, 0, 0, W}, {NULL, 0, 0, NULL, 0, 0, H}, &tab[1], &tab[2]};
    int rc;
    if ((rc = stage_decode(&S, &rule, inputs, input_sizes, boxes, status, infos, n, flags)) || (rc = lbl_axes(&J, &S, status, n)))
        goto done;
    dev_tables_place(tab, 3);
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] != DEBIG_PNG_OK) continue;
        debig_png_label_task p;
        memset(&p, 0, sizeof p);
        p.src_pitch = S.inf[i].width;
        p.out_w = W;
        p.out_h = H;
        p.src_bytes = S.inf[i].bit_depth == 16 ? 2u : 1u;
        p.dtype = (uint8_t)desc->dtype;
        if ((rc = lbl_runs(&J, &S, i, p.src_bytes, (uint64_t)H * W * es, &p))) goto done;
    }
    if (J.n_tasks == 0) goto done;
    debig_ctx *c = dev_upload(J.tasks, J.n_tasks, J.elem, tab, 3, &rc);
    if (!c) goto done;
    if ((rc = debig_hip_png_label_gather_batch(c->rsz_src.ptr, d_out, (const debig_png_label_task *)c->rsz_tasks.ptr,
                                               c->rsz_weights.ptr, desc->lut ? (const int32_t *)c->rsz_weights.ptr : NULL,
                                               (uint32_t)J.n_tasks, NULL)))
        goto done;
    rc = debig_hip_stream_sync(NULL);
done:
    stage_free(&S);
    lbl_job_free(&J);
    return rc;
}

/* ---- debig_png_decode_batch_color_labels: RGB-coded masks -> one dense integer class-map tensor (decode_png.h) --------------- */

/* the smallest table of a map of n keys (include/debig_hip.h): a power of two, >= 2 n, >= 2 */
static uint32_t cmap_slots(uint32_t n)
{
    uint32_t s = 2;
    while (s < 2u * n) s *= 2;
    return s;
}

DEBIG_API uint32_t debig_png_color_map_table(const debig_png_color_map *map, uint32_t *table, uint32_t cap_slots)
{
    if (!map || !table || map->n > DEBIG_PNG_CMAP_MAX || (map->n && (!map->keys || !map->values))) return 0;
    const uint32_t slots = cmap_slots(map->n);
    if (slots > cap_slots) return 0;
    for (uint32_t k = 0; k < map->n; k++)
        if (map->keys[k] > 0xFFFFFFu) return 0;
    /* (two equal keys are found while the table fills: it is the caller's only once it is whole) */
    uint32_t tmp[2u * DEBIG_PNG_CMAP_MAX_SLOTS];
    for (uint32_t s = 0; s < slots; s++) { tmp[2u * s] = DEBIG_PNG_CMAP_EMPTY; tmp[2u * s + 1u] = 0u; }
    for (uint32_t k = 0; k < map->n; k++) {
        const uint32_t key = map->keys[k];
        uint32_t s = DEBIG_PNG_CMAP_SLOT(key, slots);
        while (tmp[2u * s] != DEBIG_PNG_CMAP_EMPTY) { /* (n <= slots / 2: an unused slot exists) */
            if (tmp[2u * s] == key) return 0;
            s = (s + 1u) & (slots - 1u);
        }
        tmp[2u * s] = key;
        tmp[2u * s + 1u] = (uint32_t)map->values[k];
    }
    memcpy(table, tmp, (size_t)slots * 8u);
    return slots;
}

/* the maps of one call as the device takes them: the tables one behind the other, table k at off[k] bytes with slots[k] slots */
typedef struct clbl_maps {
    uint32_t *tab;
    uint64_t *off, bytes;
    uint32_t *slots;
} clbl_maps;

static void clbl_maps_free(clbl_maps *M)
{
    free(M->tab);
    free(M->off);
    free(M->slots);
}

/* the argument checks of debig_png_decode_batch_color_labels (n > 0) on their own, before any file is looked at: the label
 * call's, then the mode's and the maps'; in MAP mode the tables are made on the way (two equal keys show up there).
 * -> 0 (*M filled, the caller's to clbl_maps_free either way), DEBIG_PNG_BAD_ARG or 2 */
static int clbl_args_check(const void *d_out, const debig_png_color_label_desc *desc, uint32_t n, clbl_maps *M)
{
    if (!desc || !d_out || ((uintptr_t)d_out & 15u)) return DEBIG_PNG_BAD_ARG;
    if (desc->out_w == 0 || desc->out_w > 16384u || desc->out_h == 0 || desc->out_h > 16384u || desc->dtype > DEBIG_PNG_L_I64 ||
        desc->reserved != 0 || desc->mode > DEBIG_PNG_CL_MAP)
        return DEBIG_PNG_BAD_ARG;
    const int map_mode = desc->mode == DEBIG_PNG_CL_MAP;
    if (!map_mode && (desc->dtype < DEBIG_PNG_L_I32 || desc->n_maps != 0)) return DEBIG_PNG_BAD_ARG;
    if (map_mode && ((desc->n_maps != 1 && desc->n_maps != n) || !desc->maps)) return DEBIG_PNG_BAD_ARG;
    if (!map_mode) return 0;
    const uint32_t n_maps = desc->n_maps;
    const int64_t top = desc->dtype == DEBIG_PNG_L_U8 ? 255 : desc->dtype == DEBIG_PNG_L_U16 ? 65535 : INT32_MAX;
    const int64_t low = desc->dtype <= DEBIG_PNG_L_U16 ? 0 : INT32_MIN;
    if (desc->missing < low || desc->missing > top) return DEBIG_PNG_BAD_ARG;
    uint64_t total_slots = 0;
    for (uint32_t k = 0; k < n_maps; k++) {
        const debig_png_color_map *m = &desc->maps[k];
        if (m->n > DEBIG_PNG_CMAP_MAX || (m->n && (!m->keys || !m->values))) return DEBIG_PNG_BAD_ARG;
        for (uint32_t j = 0; j < m->n; j++)
            if (m->values[j] < low || m->values[j] > top) return DEBIG_PNG_BAD_ARG;
        total_slots += cmap_slots(m->n);
    }
    M->tab = (uint32_t *)malloc((size_t)total_slots * 8u);
    M->off = (uint64_t *)calloc(n_maps, sizeof(uint64_t));
    M->slots = (uint32_t *)calloc(n_maps, sizeof(uint32_t));
    if (!M->tab || !M->off || !M->slots) return 2;
    for (uint32_t k = 0; k < n_maps; k++) {
        M->off[k] = M->bytes;
        M->slots[k] = debig_png_color_map_table(&desc->maps[k], M->tab + M->bytes / 4u, DEBIG_PNG_CMAP_MAX_SLOTS);
        if (M->slots[k] == 0) return DEBIG_PNG_BAD_ARG; /* a key above 0xFFFFFF, or two equal keys */
        M->bytes += (uint64_t)M->slots[k] * 8u;
    }
    return 0;
}

DEBIG_API int debig_png_decode_batch_color_labels(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                  const debig_png_box *boxes, uint32_t *status, debig_png_info *infos,
                                                  uint32_t *unmatched, uint32_t n, uint32_t flags,
                                                  const debig_png_color_label_desc *desc)
{
    if (n == 0) return 0;
    clbl_maps M = {NULL, NULL, 0, NULL};
    uint32_t *cnt = NULL;
    stage S = {NULL, NULL, NULL, NULL, NULL};
    /* the maps' tables (first: map_off needs no base), the X tables, the Y tables, the counters (16-byte aligned) */
    dev_table tab[4] = {{NULL, 0, 0}, {NULL, 0, 0}, {NULL, 0, 0}, {NULL, (uint64_t)n * sizeof(uint32_t), 0}};
    lbl_job J = {NULL, 0, 0, 0, 0, sizeof(debig_png_color_label_task), offsetof(debig_png_color_label_task, row0),
                 {NULL, 0, 0, NULL, 0, 0, 0}, {NULL, 0, 0, NULL, 0, 0, 0}, &tab[1], &tab[2]};
    int rc;
    if ((rc = clbl_args_check(d_out, desc, n, &M))) goto done;
    const int map_mode = desc->mode == DEBIG_PNG_CL_MAP;
    const uint32_t W = desc->out_w, H = desc->out_h, es = 1u << desc->dtype, n_maps = map_mode ? desc->n_maps : 0;
    const stage_rule rule = {DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8, 0, 0, 1, 0, 0, NULL, NULL, NULL, NULL}; /* E_LABEL: a 16-bit file */
    J.W = J.TX.L = W;
    J.H = J.TY.L = H;
    tab[0].src = M.tab;
    tab[0].bytes = M.bytes;
    rc = 2;
    cnt = (uint32_t *)calloc(n, sizeof(uint32_t));
    if (!cnt) goto done;
    if ((rc = stage_decode(&S, &rule, inputs, input_sizes, boxes, status, infos, n, flags))) goto done;
    if (unmatched) memset(unmatched, 0, (size_t)n * sizeof(uint32_t));
    if ((rc = lbl_axes(&J, &S, status, n))) goto done;
    dev_tables_place(tab, 4);
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] != DEBIG_PNG_OK) continue;
        const uint32_t mk = n_maps == 1 ? 0u : i;
        debig_png_color_label_task p;
        memset(&p, 0, sizeof p);
        p.src_pitch = S.inf[i].width;
        p.out_w = W;
        p.out_h = H;
        p.dtype = (uint8_t)desc->dtype;
        p.mode = (uint8_t)desc->mode;
        p.image = i;
        if (map_mode) {
            p.map_off = tab[0].off + M.off[mk];
            p.map_slots = M.slots[mk];
            p.missing = desc->missing;
        }
        if ((rc = lbl_runs(&J, &S, i, 3u, (uint64_t)H * W * es, &p))) goto done;
    }
    if (J.n_tasks == 0) goto done;
    debig_ctx *c = dev_upload(J.tasks, J.n_tasks, J.elem, tab, 4, &rc);
    if (!c) goto done;
    uint32_t *d_cnt = map_mode ? (uint32_t *)((uint8_t *)c->rsz_weights.ptr + tab[3].off) : NULL;
    if ((d_cnt && (rc = debig_hip_memset(d_cnt, 0, tab[3].bytes, NULL))) ||
        (rc = debig_hip_png_color_label_batch(c->rsz_src.ptr, d_out, (const debig_png_color_label_task *)c->rsz_tasks.ptr,
                                              c->rsz_weights.ptr, d_cnt, (uint32_t)J.n_tasks, NULL)) ||
        (d_cnt && (rc = debig_hip_memcpy_d2h(cnt, d_cnt, tab[3].bytes, NULL))) ||
        (rc = debig_hip_stream_sync(NULL)))
        goto done;
    if (unmatched && map_mode) memcpy(unmatched, cnt, (size_t)n * sizeof(uint32_t));
done:
    clbl_maps_free(&M);
    free(cnt);
    stage_free(&S);
    lbl_job_free(&J);
    return rc;
}

/* ---- what the calls that post-process a dense (n, h, w) label tensor share: stats, boundary, distance, components ---------------- */

#define LABEL_POST_NO_OUT UINT32_MAX

/* the tensor arguments of such a call: labels of a known dtype, aligned to their element, sides of 1 .. 16384; and, unless
 * out_shift is LABEL_POST_NO_OUT, a device output of 1 << out_shift bytes per element, aligned to that and apart from the input.
 * (out_shift is read behind the dtype test, so a caller may hand in the dtype itself.)  -> 1, or 0: DEBIG_PNG_BAD_ARG */
static int label_post_args_ok(const void *d_labels, const void *d_out, uint32_t out_shift, uint32_t n, uint32_t w, uint32_t h, uint32_t dtype)
{
    if (!d_labels || dtype > DEBIG_PNG_L_I64 || w == 0 || w > 16384u || h == 0 || h > 16384u) return 0;
    const uint64_t es = 1u << dtype, elems = (uint64_t)n * w * h;
    if ((uintptr_t)d_labels & (es - 1u)) return 0;
    if (out_shift == LABEL_POST_NO_OUT) return 1;
    const uint64_t os = 1u << out_shift;
    if (!d_out || ((uintptr_t)d_out & (os - 1u))) return 0;
    return !((uintptr_t)d_out < (uintptr_t)d_labels + elems * es && (uintptr_t)d_labels < (uintptr_t)d_out + elems * os);
}

/* the GOOD images, those the call looks at (no status, or an entry of 0): *i moves on to the first one at or behind it -> 0: there
 * is none.  for (i = 0, k = 0; label_post_good(status, n, &i); i++, k++) visits them all, k the image's place among them. */
static int label_post_good(const uint32_t *status, uint32_t n, uint32_t *i)
{
    while (*i < n && status && status[*i] != 0) (*i)++;
    return *i < n;
}

static uint64_t label_post_n_good(const uint32_t *status, uint32_t n)
{
    uint64_t n_good = 0;
    for (uint32_t i = 0; label_post_good(status, n, &i); i++) n_good++;
    return n_good;
}

/* per tasks for each of n_good images: does a launch take them?  (0: the call returns 2) */
static int label_post_tasks_fit(uint64_t n_good, uint64_t per) { return n_good * per < 0x7fffffffu; }

/* ---- debig_png_label_stats: per-id counts and bounding boxes of a dense label tensor (decode_png.h) -------------------------- */

_Static_assert(sizeof(debig_png_label_stat) == 20 && sizeof(debig_png_label_box) == 20 && sizeof(debig_png_label_stats_task) == 40,
               "the raw record is five uint32, and so is the public one");

DEBIG_API void debig_png_label_stat_box(const uint32_t raw[5], uint32_t out_w, uint32_t out_h, debig_png_label_box *box)
{
    memset(box, 0, sizeof *box);
    if (raw[0] == 0) return; /* the id does not occur: the extremes of an empty record mean nothing */
    box->count = raw[0];
    box->x0 = out_w - raw[3];
    box->y0 = out_h - raw[4];
    box->x1 = raw[1];
    box->y1 = raw[2];
}

DEBIG_API int debig_png_label_stats(const void *d_labels, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype, uint32_t n_ids,
                                    const uint32_t *status, debig_png_label_box *out)
{
    if (n == 0) return 0;
    if (!out || n_ids == 0 || n_ids > DEBIG_PNG_LABEL_STATS_MAX_IDS ||
        !label_post_args_ok(d_labels, NULL, LABEL_POST_NO_OUT, n, out_w, out_h, dtype))
        return DEBIG_PNG_BAD_ARG;
    const uint32_t es = 1u << dtype, recs = n_ids + 1u;
    const uint32_t run = row_run(out_w, LBL_TASK_ELEMS), per = (out_h + run - 1u) / run;
    const uint64_t n_good = label_post_n_good(status, n);
    if (!label_post_tasks_fit(n_good, per)) return 2;
    memset(out, 0, (size_t)n * recs * sizeof *out);
    if (n_good == 0) return 0;
    int rc = 2;
    debig_png_label_stats_task *tasks = (debig_png_label_stats_task *)malloc((size_t)(n_good * per) * sizeof *tasks);
    dev_table tab[1] = {{NULL, (uint64_t)n * recs * sizeof(debig_png_label_stat), 0}}; /* the raw records: space only */
    uint32_t *raw = (uint32_t *)malloc((size_t)tab[0].bytes);
    uint64_t n_tasks = 0;
    if (!tasks || !raw) goto done;
    for (uint32_t i = 0; label_post_good(status, n, &i); i++) {
        for (uint32_t y0 = 0; y0 < out_h; y0 += run) {
            debig_png_label_stats_task *t = &tasks[n_tasks++];
            t->label_off = ((uint64_t)i * out_h + y0) * out_w * es;
            t->stat_off = (uint64_t)i * recs * sizeof(debig_png_label_stat);
            t->out_w = out_w;
            t->out_h = out_h;
            t->row0 = y0;
            t->rows = run_rows(out_h, y0, run);
            t->n_ids = n_ids;
            t->dtype = dtype;
        }
    }
    debig_ctx *c = dev_upload(tasks, n_tasks, sizeof *tasks, tab, 1, &rc);
    if (!c) goto done;
    if ((rc = debig_hip_memset(c->rsz_weights.ptr, 0, tab[0].bytes, NULL)) ||
        (rc = debig_hip_png_label_stats_batch(d_labels, c->rsz_weights.ptr, (const debig_png_label_stats_task *)c->rsz_tasks.ptr,
                                              (uint32_t)n_tasks, NULL)) ||
        (rc = debig_hip_memcpy_d2h(raw, c->rsz_weights.ptr, tab[0].bytes, NULL)) || (rc = debig_hip_stream_sync(NULL)))
        goto done;
    for (uint64_t k = 0; k < (uint64_t)n * recs; k++) debig_png_label_stat_box(raw + 5u * k, out_w, out_h, &out[k]);
done:
    free(tasks);
    free(raw);
    return rc;
}

/* ---- debig_png_label_boundary: ignore rings and edge maps of a dense label tensor (decode_png.h) -------------------------------- */

_Static_assert(sizeof(debig_png_label_boundary_task) == 80 && offsetof(debig_png_label_boundary_task, reach) == 60,
               "three 64-bit fields, nine uint32, the reach table, padded to a multiple of 8");

DEBIG_API void debig_png_label_boundary_reach(uint32_t radius, uint32_t shape, uint8_t reach[17])
{
    memset(reach, 0, 17);
    if (radius > DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS || shape > DEBIG_PNG_BOUNDARY_DISK) return;
    for (uint32_t d = 0; d <= radius; d++) {
        uint32_t v = radius;
        if (shape == DEBIG_PNG_BOUNDARY_DIAMOND) v = radius - d;
        if (shape == DEBIG_PNG_BOUNDARY_DISK) /* the largest v with v * v + d * d <= radius * radius */
            while (v * v + d * d > radius * radius) v--;
        reach[d] = (uint8_t)v;
    }
}

/* the tile of the call: the largest of 128 x 64, 64 x 64, 64 x 32, 32 x 32 whose planes fit the kernel's LDS */
static void boundary_tile(uint32_t dtype, uint32_t radius, uint32_t *tw, uint32_t *th)
{
    *tw = 128u;
    *th = 64u;
    while (DEBIG_PNG_LABEL_BOUNDARY_TILE_BYTES(*tw, *th, dtype, radius) > DEBIG_PNG_LABEL_BOUNDARY_LDS_BYTES) {
        if (*tw > *th) *tw /= 2u;
        else *th /= 2u;
    }
}

DEBIG_API int debig_png_label_boundary(const void *d_labels, void *d_out, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype,
                                       uint32_t radius, uint32_t shape, uint32_t mode, int64_t value, const uint32_t *status)
{
    if (n == 0) return 0;
    if (radius == 0 || radius > DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS || shape > DEBIG_PNG_BOUNDARY_DISK || mode > DEBIG_PNG_BOUNDARY_EDGE ||
        !label_post_args_ok(d_labels, d_out, mode == DEBIG_PNG_BOUNDARY_RING ? dtype : 0u, n, out_w, out_h, dtype))
        return DEBIG_PNG_BAD_ARG;
    if (mode == DEBIG_PNG_BOUNDARY_RING &&
        ((dtype == DEBIG_PNG_L_U8 && (value < 0 || value > 255)) || (dtype == DEBIG_PNG_L_U16 && (value < 0 || value > 65535)) ||
         (dtype == DEBIG_PNG_L_I32 && (value < INT32_MIN || value > INT32_MAX))))
        return DEBIG_PNG_BAD_ARG;
    const uint32_t es = 1u << dtype, os = mode == DEBIG_PNG_BOUNDARY_RING ? es : 1u;
    const uint64_t img = (uint64_t)out_w * out_h;
    uint32_t tw, th;
    boundary_tile(dtype, radius, &tw, &th);
    const uint64_t per = (uint64_t)((out_w + tw - 1u) / tw) * ((out_h + th - 1u) / th);
    const uint64_t n_good = label_post_n_good(status, n);
    if (!label_post_tasks_fit(n_good, per)) return 2;
    if (n_good == 0) return 0;
    int rc = 2;
    debig_png_label_boundary_task *tasks = (debig_png_label_boundary_task *)calloc((size_t)(n_good * per), sizeof *tasks);
    dev_table tab[1] = {{NULL, 0, 0}}; /* no tables */
    uint64_t n_tasks = 0;
    if (!tasks) goto done;
    for (uint32_t i = 0; label_post_good(status, n, &i); i++) {
        for (uint32_t y0 = 0; y0 < out_h; y0 += th)
            for (uint32_t x0 = 0; x0 < out_w; x0 += tw) {
                debig_png_label_boundary_task *t = &tasks[n_tasks++];
                t->label_off = (uint64_t)i * img * es;
                t->out_off = (uint64_t)i * img * os;
                t->value = value;
                t->w = out_w;
                t->h = out_h;
                t->x0 = x0;
                t->y0 = y0;
                t->tile_w = out_w - x0 < tw ? out_w - x0 : tw;
                t->tile_h = out_h - y0 < th ? out_h - y0 : th;
                t->dtype = dtype;
                t->mode = mode;
                t->radius = radius;
                debig_png_label_boundary_reach(radius, shape, t->reach);
            }
    }
    debig_ctx *c = dev_upload(tasks, n_tasks, sizeof *tasks, tab, 1, &rc);
    if (!c) goto done;
    if ((rc = debig_hip_png_label_boundary_batch(d_labels, d_out, (const debig_png_label_boundary_task *)c->rsz_tasks.ptr, (uint32_t)n_tasks,
                                                 NULL)))
        goto done;
    rc = debig_hip_stream_sync(NULL);
done:
    free(tasks);
    return rc;
}

/* ---- debig_png_label_distance: exact squared Euclidean distance maps of a dense label tensor (decode_png.h) --------------------- */

_Static_assert(sizeof(debig_png_label_distance_rows_task) == 48 && offsetof(debig_png_label_distance_rows_task, w) == 24,
               "three 64-bit fields, six uint32");
_Static_assert(sizeof(debig_png_label_distance_cols_task) == 40 && offsetof(debig_png_label_distance_cols_task, w) == 16,
               "two 64-bit fields, six uint32");

DEBIG_API int debig_png_label_distance(const void *d_labels, void *d_out, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype,
                                       uint32_t sites, int64_t value, uint32_t cap, uint32_t format, const uint32_t *status)
{
    if (n == 0) return 0;
    if (sites > DEBIG_PNG_DISTANCE_TO_VALUE || format > DEBIG_PNG_DISTANCE_ROOT || cap > DEBIG_PNG_LABEL_DISTANCE_MAX_CAP ||
        !label_post_args_ok(d_labels, d_out, 2u, n, out_w, out_h, dtype))
        return DEBIG_PNG_BAD_ARG;
    const uint32_t es = 1u << dtype;
    const uint64_t img = (uint64_t)out_w * out_h;
    /* a rows task: a run of whole rows of at most DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS elements; a cols task: a strip of 64 columns */
    const uint32_t run = row_run(out_w, DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS);
    const uint64_t per_r = (out_h + run - 1u) / run, per_c = (out_w + DEBIG_PNG_LABEL_DISTANCE_COLS - 1u) / DEBIG_PNG_LABEL_DISTANCE_COLS;
    const uint64_t n_good = label_post_n_good(status, n);
    if (!label_post_tasks_fit(n_good, per_r) || !label_post_tasks_fit(n_good, per_c)) return 2;
    if (n_good == 0) return 0;
    int rc = 2;
    /* both task lists in one upload: the rows tasks, the cols tasks behind them (48 is a multiple of 8) */
    const uint64_t n_r = n_good * per_r, n_c = n_good * per_c;
    const uint64_t bytes = n_r * sizeof(debig_png_label_distance_rows_task) + n_c * sizeof(debig_png_label_distance_cols_task);
    uint8_t *blob = (uint8_t *)calloc((size_t)bytes, 1);
    dev_table tab[1] = {{NULL, n_good * img * 2u, 0}}; /* the g planes of the images that are looked at: space only */
    if (!blob) goto done;
    debig_png_label_distance_rows_task *tr = (debig_png_label_distance_rows_task *)blob;
    debig_png_label_distance_cols_task *tc = (debig_png_label_distance_cols_task *)(blob + n_r * sizeof *tr);
    for (uint32_t i = 0, k = 0; label_post_good(status, n, &i); i++, k++) {
        for (uint32_t y0 = 0; y0 < out_h; y0 += run, tr++) {
            tr->label_off = (uint64_t)i * img * es;
            tr->g_off = k * img * 2u;
            tr->value = value;
            tr->w = out_w;
            tr->h = out_h;
            tr->row0 = y0;
            tr->rows = run_rows(out_h, y0, run);
            tr->dtype = dtype;
            tr->sites = sites;
        }
        for (uint32_t x0 = 0; x0 < out_w; x0 += DEBIG_PNG_LABEL_DISTANCE_COLS, tc++) {
            tc->g_off = k * img * 2u;
            tc->out_off = (uint64_t)i * img * 4u;
            tc->w = out_w;
            tc->h = out_h;
            tc->x0 = x0;
            tc->cols = out_w - x0 < DEBIG_PNG_LABEL_DISTANCE_COLS ? out_w - x0 : DEBIG_PNG_LABEL_DISTANCE_COLS;
            tc->cap = cap;
            tc->format = format;
        }
    }
    debig_ctx *c = dev_upload(blob, bytes, 1, tab, 1, &rc);
    if (!c) goto done;
    const uint8_t *d_tasks = (const uint8_t *)c->rsz_tasks.ptr;
    if ((rc = debig_hip_png_label_distance_rows_batch(d_labels, c->rsz_weights.ptr, (const debig_png_label_distance_rows_task *)d_tasks,
                                                      (uint32_t)n_r, NULL)) ||
        (rc = debig_hip_png_label_distance_cols_batch(c->rsz_weights.ptr,
                                                      d_out, (const debig_png_label_distance_cols_task *)(d_tasks + n_r * sizeof *tr),
                                                      (uint32_t)n_c, NULL)))
        goto done;
    rc = debig_hip_stream_sync(NULL);
done:
    free(blob);
    return rc;
}

/* ---- debig_png_label_components: connected components of a dense label tensor (decode_png.h) ------------------------------------- */

_Static_assert(sizeof(debig_png_label_components_task) == 80 && offsetof(debig_png_label_components_task, w) == 32,
               "four 64-bit fields, twelve uint32");

DEBIG_API int debig_png_label_components(const void *d_labels, void *d_out, uint32_t n, uint32_t out_w, uint32_t out_h, uint32_t dtype,
                                         uint32_t connectivity, uint32_t use_background, int64_t background, uint32_t ids,
                                         const uint32_t *status, uint32_t *counts)
{
    if (n == 0) return 0;
    if ((connectivity != 4u && connectivity != 8u) || ids > DEBIG_PNG_COMPONENTS_CONSECUTIVE ||
        !label_post_args_ok(d_labels, d_out, 2u, n, out_w, out_h, dtype))
        return DEBIG_PNG_BAD_ARG;
    const uint32_t es = 1u << dtype;
    const uint64_t img = (uint64_t)out_w * out_h;
    if (counts) memset(counts, 0, (size_t)n * sizeof *counts);
    /* a task: a run of whole rows of at most DEBIG_PNG_LABEL_COMPONENTS_ELEMS elements, the same cut for all five launches */
    const uint32_t run = row_run(out_w, DEBIG_PNG_LABEL_COMPONENTS_ELEMS);
    const uint64_t per = (out_h + run - 1u) / run;
    const uint64_t n_good = label_post_n_good(status, n);
    if (!label_post_tasks_fit(n_good, per)) return 2;
    if (n_good == 0) return 0;
    int rc = 2;
    const uint64_t n_tasks = n_good * per;
    debig_png_label_components_task *tasks = (debig_png_label_components_task *)calloc((size_t)n_tasks, sizeof *tasks), *t = tasks;
    uint32_t *task_counts = (uint32_t *)malloc((size_t)n_tasks * sizeof *task_counts);
    /* the parent planes of the images that are looked at, the tasks' counts behind them: space only */
    dev_table tab[2] = {{NULL, n_good * img * 4u, 0}, {NULL, n_tasks * sizeof(uint32_t), 0}};
    dev_tables_place(tab, 2);
    if (!tasks || !task_counts) goto done;
    for (uint32_t i = 0, k = 0; label_post_good(status, n, &i); i++, k++) {
        for (uint32_t y0 = 0; y0 < out_h; y0 += run, t++) {
            t->label_off = (uint64_t)i * img * es;
            t->parent_off = k * img * 4u;
            t->out_off = (uint64_t)i * img * 4u;
            t->background = background;
            t->w = out_w;
            t->h = out_h;
            t->row0 = y0;
            t->rows = run_rows(out_h, y0, run);
            t->dtype = dtype;
            t->connectivity = connectivity;
            t->use_background = use_background != 0;
            t->ids = ids;
            t->count_first = (uint32_t)(k * per);
            t->count_idx = (uint32_t)(t - tasks);
        }
    }
    debig_ctx *c = dev_upload(tasks, n_tasks, sizeof *tasks, tab, 2, &rc);
    if (!c) goto done;
    const debig_png_label_components_task *d_tasks = (const debig_png_label_components_task *)c->rsz_tasks.ptr;
    void *d_parent = c->rsz_weights.ptr, *d_counts = (uint8_t *)c->rsz_weights.ptr + tab[1].off;
    if ((rc = debig_hip_png_label_components_rows_batch(d_labels, d_parent, d_tasks, (uint32_t)n_tasks, NULL)) ||
        (rc = debig_hip_png_label_components_merge_batch(d_labels, d_parent, d_tasks, (uint32_t)n_tasks, NULL)) ||
        (rc = debig_hip_png_label_components_count_batch(d_parent, d_counts, d_tasks, (uint32_t)n_tasks, NULL)) ||
        (ids == DEBIG_PNG_COMPONENTS_CONSECUTIVE &&
         (rc = debig_hip_png_label_components_number_batch(d_parent, d_counts, d_out, d_tasks, (uint32_t)n_tasks, NULL))) ||
        (rc = debig_hip_png_label_components_finish_batch(d_parent, d_out, d_tasks, (uint32_t)n_tasks, NULL)) ||
        (rc = debig_hip_memcpy_d2h(task_counts, d_counts, tab[1].bytes, NULL)) || (rc = debig_hip_stream_sync(NULL)))
        goto done;
    if (counts)
        for (uint32_t i = 0, k = 0; label_post_good(status, n, &i); i++, k++)
            for (uint64_t j = 0; j < per; j++) counts[i] += task_counts[k * per + j];
done:
    free(tasks);
    free(task_counts);
    return rc;
}

/* ---- the affine warp of the tensor and the label decode (decode_png.h) ------------------------------------------------------ */

#define WARP_TASK_PIXELS 4096u /* output pixels of one warp task (a run of whole rows; one row when it is wider): 16 per lane */

DEBIG_API int debig_png_warp_quantise(const double M[6], int64_t m[6])
{
    for (uint32_t k = 0; k < 6; k++) {
        uint64_t u;
        memcpy(&u, &M[k], 8);
        if ((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return 0; /* infinity or NaN */
        const double lim = k == 2 || k == 5 ? 16777216.0 : 32768.0, a = M[k] < 0 ? -M[k] : M[k];
        if (a > lim) return 0;
        /* llround: the product is exact (a power of two) and below 2^41, so is x - trunc(x); halves go away from zero */
        const double x = M[k] * 65536.0;
        int64_t q = (int64_t)x;
        const double d = x - (double)q;
        if (d >= 0.5) q++;
        else if (d <= -0.5) q--;
        m[k] = q;
    }
    return 1;
}

DEBIG_API int debig_png_persp_quantise(const double M[9], int64_t m[9])
{
    if (!debig_png_warp_quantise(M, m)) return 0; /* rows 0 and 1: the affine quantiser, its limits and its rounding */
    for (uint32_t k = 6; k < 9; k++) {
        uint64_t u;
        memcpy(&u, &M[k], 8);
        if ((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return 0; /* infinity or NaN */
        if ((M[k] < 0 ? -M[k] : M[k]) > 4.0) return 0;
        /* llround: the product is exact (a power of two) and at most 2^32, so is x - trunc(x); halves go away from zero */
        const double x = M[k] * 1073741824.0;
        int64_t q = (int64_t)x;
        const double d = x - (double)q;
        if (d >= 0.5) q++;
        else if (d <= -0.5) q--;
        m[k] = q;
    }
    return 1;
}

DEBIG_API int debig_png_persp_range(const int64_t m[9], uint32_t out_w, uint32_t out_h)
{
    if (out_w == 0 || out_w > 16384u || out_h == 0 || out_h > 16384u) return 0;
    for (uint32_t k = 6; k < 9; k++)
        if (m[k] < -((int64_t)1 << 32) || m[k] > ((int64_t)1 << 32)) return 0;
    /* D is linear in X and Y: its extremes lie at the corner pixels (|D| < 2^49 there) */
    for (uint32_t k = 0; k < 4; k++) {
        const int64_t cx = k & 1u ? 2 * (int64_t)out_w - 1 : 1, cy = k & 2u ? 2 * (int64_t)out_h - 1 : 1;
        const int64_t D = m[6] * cx + m[7] * cy + 2 * m[8];
        if (D < ((int64_t)1 << 21) || D > ((int64_t)1 << 33) - 1) return 0;
    }
    return 1;
}

/* ---- the elastic deformation of the three warp calls (decode_png.h has the rule; csrc/png_elastic_kernel.inc restates it) ------- */

DEBIG_API int debig_png_elastic_quantise(const double *v, uint64_t count, int32_t *q)
{
    for (uint64_t k = 0; k < count; k++) {
        uint64_t u;
        memcpy(&u, &v[k], 8);
        if ((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return 0; /* infinity or NaN */
        if ((v[k] < 0 ? -v[k] : v[k]) > 4096.0) return 0;
        q[k] = (int32_t)color_llround(v[k] * 65536.0); /* (the product is exact: a power of two; at most 2^28) */
    }
    return 1;
}

DEBIG_API void debig_png_elastic_cell(uint32_t X, uint32_t W, uint32_t g, uint32_t *k, uint32_t *t)
{
    const uint32_t num = (2u * X + 1u) * (g - 1u), den = 2u * W;
    *k = num / den;
    *t = ((num - *k * den) * 16384u + W) / den;
}

DEBIG_API void debig_png_elastic_weights(uint32_t t, int32_t w[4])
{
    const int64_t T = (int64_t)t, t2 = T * T, t3 = t2 * T, half = (int64_t)1 << 28;
    /* (>> of a negative int64 is an arithmetic shift with gcc and clang, which build this file) */
    w[0] = (int32_t)((-t3 + 2 * t2 * 16384 - T * ((int64_t)1 << 28) + half) >> 29);
    w[1] = (int32_t)((3 * t3 - 5 * t2 * 16384 + ((int64_t)1 << 43) + half) >> 29);
    w[2] = (int32_t)((-3 * t3 + 4 * t2 * 16384 + T * ((int64_t)1 << 28) + half) >> 29);
    w[3] = (int32_t)((t3 - t2 * 16384 + half) >> 29);
    if (t < 8192u) w[1] = 16384 - (w[0] + w[2] + w[3]);
    else w[2] = 16384 - (w[0] + w[1] + w[3]);
}

DEBIG_API int debig_png_elastic_displacement(const int32_t *q, uint32_t grid_w, uint32_t grid_h, uint32_t out_w, uint32_t out_h,
                                             uint32_t X, uint32_t Y, int64_t *Dx, int64_t *Dy)
{
    if (!q || grid_w < 2 || grid_w > 33 || grid_h < 2 || grid_h > 33 || out_w == 0 || out_w > 16384u || out_h == 0 ||
        out_h > 16384u || X >= out_w || Y >= out_h)
        return 0;
    uint32_t kx, tx, ky, ty;
    int32_t wx[4], wy[4];
    debig_png_elastic_cell(X, out_w, grid_w, &kx, &tx);
    debig_png_elastic_cell(Y, out_h, grid_h, &ky, &ty);
    debig_png_elastic_weights(tx, wx);
    debig_png_elastic_weights(ty, wy);
    int64_t sx = 0, sy = 0;
    for (uint32_t i = 0; i < 4; i++) {
        const int64_t r = (int64_t)ky - 1 + i, ry = r < 0 ? 0 : r > (int64_t)grid_h - 1 ? (int64_t)grid_h - 1 : r;
        for (uint32_t j = 0; j < 4; j++) {
            const int64_t c = (int64_t)kx - 1 + j, cx = c < 0 ? 0 : c > (int64_t)grid_w - 1 ? (int64_t)grid_w - 1 : c;
            const int32_t *d = q + 2 * (ry * grid_w + cx);
            if (d[0] < -(1 << 28) || d[0] > (1 << 28) || d[1] < -(1 << 28) || d[1] > (1 << 28)) return 0;
            sx += (int64_t)wy[i] * wx[j] * d[0];
            sy += (int64_t)wy[i] * wx[j] * d[1];
        }
    }
    *Dx = (sx + ((int64_t)1 << 27)) >> 28;
    *Dy = (sy + ((int64_t)1 << 27)) >> 28;
    return 1;
}

#define MAP_INTS 9u /* a file's quantised map: m[0..5] (every kind), m[6..8] = p[] (the projective kind; else unused) */
#define ELA_TAIL 16u /* what an elastic task adds to its warp task: field_off, grid_w, grid_h, a reserved word */

/* the map of one warp call: its kind and the caller's arrays (warps: affine and elastic; persps: projective; elastics and ed:
 * elastic); behind map_prepare the files' quantised maps (MAP_INTS int64 each) and their E_WARP flags, and of an elastic call the
 * quantised nodes of all files (rec bytes each, zeros where a file has none) and, behind map_place, where they land in
 * c->rsz_weights.  A new map is a kind here, an arm in map_prepare, map_tail_bytes and map_task_runs and one in each map_launch_* */
typedef enum map_kind { MAP_AFFINE, MAP_PERSP, MAP_ELASTIC } map_kind;
typedef struct warp_map {
    map_kind kind;
    const debig_png_warp *warps;
    const debig_png_persp *persps;
    const debig_png_elastic *elastics;
    const debig_png_elastic_desc *ed;
    int64_t *m;
    uint8_t *bad;
    int32_t *q;
    uint64_t rec, off;
} warp_map;

/* the map of a call as its public entry point makes it (a compound literal: it lives until the entry point returns) */
#define MAP_OF(kind_, ...) (&(warp_map){.kind = kind_, __VA_ARGS__})

/* the caller's array of per-file matrices (NULL: not given) */
static const void *map_given(const warp_map *mp) { return mp->kind == MAP_PERSP ? (const void *)mp->persps : (const void *)mp->warps; }

/* what a task of this map adds to its warp task */
static size_t map_tail_bytes(const warp_map *mp) { return mp->kind == MAP_PERSP ? 3 * sizeof(int64_t) : mp->kind == MAP_ELASTIC ? ELA_TAIL : 0; }

/* check and prepare, behind every check of the affine call: the elastic arguments (-> DEBIG_PNG_BAD_ARG), then the files' maps
 * quantised and flagged -- projective: the D range over the out_w x out_h output is part of the flag; elastic: the fields
 * quantised as well, a node out of range part of the flag -> 0, DEBIG_PNG_BAD_ARG or 2 */
static int map_prepare(warp_map *mp, uint32_t n, uint32_t out_w, uint32_t out_h)
{
    const debig_png_elastic_desc *ed = mp->ed;
    size_t per = 0; /* the int32 of one field */
    if (mp->kind == MAP_ELASTIC) {
        if (!mp->elastics || !ed || ed->grid_w < 2 || ed->grid_w > 33 || ed->grid_h < 2 || ed->grid_h > 33 || ed->reserved[0] != 0 ||
            ed->reserved[1] != 0)
            return DEBIG_PNG_BAD_ARG;
        per = (size_t)ed->grid_w * ed->grid_h * 2u;
        mp->rec = per * sizeof(int32_t);
        if (!(mp->q = (int32_t *)calloc((size_t)n * per, sizeof(int32_t)))) return 2;
    }
    mp->m = (int64_t *)calloc((size_t)n * MAP_INTS, sizeof(int64_t));
    mp->bad = (uint8_t *)calloc(n, 1);
    if (!mp->m || !mp->bad) return 2;
    for (uint32_t i = 0; i < n; i++) {
        int64_t *mi = mp->m + MAP_INTS * (size_t)i;
        mp->bad[i] = mp->kind == MAP_PERSP ? !(debig_png_persp_quantise(mp->persps[i].m, mi) && debig_png_persp_range(mi, out_w, out_h))
                                           : !debig_png_warp_quantise(mp->warps[i].m, mi);
        if (per && mp->elastics[i].nodes && !debig_png_elastic_quantise(mp->elastics[i].nodes, per, mp->q + (size_t)i * per))
            mp->bad[i] = 1;
    }
    return 0;
}

static void map_release(warp_map *mp) { free(mp->m); free(mp->bad); free(mp->q); }

/* the elastic fields as the last table of a launch (no other map has a table): its offset rounded up to the 8 bytes a node takes */
static void map_place(warp_map *mp, dev_table *t, uint32_t n)
{
    if (mp->kind != MAP_ELASTIC) return;
    t->src = mp->q;
    t->bytes = (uint64_t)n * mp->rec;
    mp->off = t->off = (t->off + 7u) & ~(uint64_t)7u;
}

/* the host array of a call's tasks: `base` bytes of warp task and the map's tail each */
typedef struct map_tasks {
    uint8_t *v;
    uint64_t n;
    uint32_t cap;
    size_t base, elem;
} map_tasks;

/* the tasks of file i: the prototype `task` (base bytes; row0 and rows point into it) once per run of `run` of the H output rows,
 * each followed by p[] where the map is projective, or by the place of the file's field and the grid size where it is elastic
 * -> 0: no memory, or too many tasks */
static int map_task_runs(map_tasks *T, const warp_map *mp, const void *task, uint32_t *row0, uint32_t *rows, uint32_t H, uint32_t run,
                         uint32_t i)
{
    for (uint32_t y0 = 0; y0 < H; y0 += run) {
        if (T->n >= 0x7fffffffu || !grow((void **)&T->v, &T->cap, (uint32_t)T->n, T->elem)) return 0;
        uint8_t *at = T->v + T->n++ * T->elem;
        *row0 = y0;
        *rows = run_rows(H, y0, run);
        memcpy(at, task, T->base);
        if (mp->kind == MAP_PERSP) memcpy(at + T->base, mp->m + MAP_INTS * (size_t)i + 6, 3 * sizeof(int64_t));
        if (mp->kind == MAP_ELASTIC) {
            const uint64_t off = mp->elastics[i].nodes ? mp->off + (uint64_t)i * mp->rec : UINT64_MAX;
            const uint16_t g[4] = {(uint16_t)mp->ed->grid_w, (uint16_t)mp->ed->grid_h, 0, 0};
            memcpy(at + T->base, &off, 8);
            memcpy(at + T->base + 8, g, 8);
        }
    }
    return 1;
}

_Static_assert(offsetof(debig_png_warp_color_task, color_off) == sizeof(debig_png_warp_task) &&
                   offsetof(debig_png_warp_color_task, b) == offsetof(debig_png_warp_task, b) &&
                   offsetof(debig_png_warp_color_task, border) == offsetof(debig_png_warp_task, border) &&
                   sizeof(debig_png_warp_color_task) == 160,
               "debig_png_warp_color_task starts with debig_png_warp_task, field for field");
_Static_assert(offsetof(debig_png_persp_task, p) == sizeof(debig_png_warp_task) && sizeof(debig_png_persp_task) == 176 &&
                   offsetof(debig_png_persp_task, b) == offsetof(debig_png_warp_task, b) &&
                   offsetof(debig_png_persp_color_task, p) == sizeof(debig_png_warp_color_task) &&
                   offsetof(debig_png_persp_color_task, color_off) == offsetof(debig_png_warp_color_task, color_off) &&
                   sizeof(debig_png_persp_color_task) == 184 &&
                   offsetof(debig_png_label_persp_task, p) == sizeof(debig_png_label_warp_task) &&
                   offsetof(debig_png_label_persp_task, border_mode) == offsetof(debig_png_label_warp_task, border_mode) &&
                   sizeof(debig_png_label_persp_task) == 128 &&
                   offsetof(debig_png_color_label_persp_task, p) == sizeof(debig_png_color_label_warp_task) &&
                   offsetof(debig_png_color_label_persp_task, border_mode) == offsetof(debig_png_color_label_warp_task, border_mode) &&
                   sizeof(debig_png_color_label_persp_task) == 144,
               "each persp task is the warp task of its kernel, field for field, followed by p[3]");
_Static_assert(offsetof(debig_png_elastic_task, field_off) == sizeof(debig_png_warp_task) &&
                   offsetof(debig_png_elastic_task, grid_w) == sizeof(debig_png_warp_task) + 8 &&
                   sizeof(debig_png_elastic_task) == sizeof(debig_png_warp_task) + ELA_TAIL &&
                   offsetof(debig_png_elastic_task, b) == offsetof(debig_png_warp_task, b) &&
                   offsetof(debig_png_elastic_color_task, field_off) == sizeof(debig_png_warp_color_task) &&
                   offsetof(debig_png_elastic_color_task, color_off) == offsetof(debig_png_warp_color_task, color_off) &&
                   sizeof(debig_png_elastic_color_task) == sizeof(debig_png_warp_color_task) + ELA_TAIL &&
                   offsetof(debig_png_label_elastic_task, field_off) == sizeof(debig_png_label_warp_task) &&
                   offsetof(debig_png_label_elastic_task, border_mode) == offsetof(debig_png_label_warp_task, border_mode) &&
                   sizeof(debig_png_label_elastic_task) == sizeof(debig_png_label_warp_task) + ELA_TAIL &&
                   offsetof(debig_png_color_label_elastic_task, field_off) == sizeof(debig_png_color_label_warp_task) &&
                   offsetof(debig_png_color_label_elastic_task, border_mode) == offsetof(debig_png_color_label_warp_task, border_mode) &&
                   sizeof(debig_png_color_label_elastic_task) == sizeof(debig_png_color_label_warp_task) + ELA_TAIL,
               "each elastic task is the warp task of its kernel, field for field, followed by field_off and the grid size");

/* the checks of debig_png_decode_batch_tensor_warp (n > 0): those of debig_png_decode_batch_tensor first and unchanged, then the
 * warp's; all before any file is looked at -> 0 or the call's return value */
static int tensor_warp_check(const void *d_out, const void *warps /* or the persps */, const debig_png_tensor_desc *desc,
                             const debig_png_warp_desc *wd)
{
    const int badarg = tensor_args_check(d_out, desc);
    if (badarg) return badarg;
    if (!warps || !wd || (wd->filter != DEBIG_PNG_FILTER_BILINEAR && wd->filter != DEBIG_PNG_FILTER_NEAREST) ||
        wd->border_mode > DEBIG_PNG_BORDER_CLAMP || wd->alpha_mode != DEBIG_PNG_ALPHA_STRAIGHT || wd->reserved != 0 ||
        desc->resize_flags != 0)
        return DEBIG_PNG_BAD_ARG;
    const uint32_t fmt = desc->out_format, ch = fmt_channels(fmt), bits = fmt & DEBIG_PNG_FMT_16 ? 16u : 8u;
    if (wd->border_mode == DEBIG_PNG_BORDER_CONSTANT)
        for (uint32_t k = 0; k < ch; k++)
            if (wd->border[k] > (1u << bits) - 1u) return DEBIG_PNG_BAD_ARG;
    return 0;
}

/* the launch of the image kind under the call's map; rec: the colour records are given, and the tasks are the colour kernel's */
static int map_launch_image(const warp_map *mp, const void *rec, const debig_ctx *c, void *out, const void *t, uint32_t cnt)
{
    const uint8_t *src = c->rsz_src.ptr, *w = c->rsz_weights.ptr;
    switch (mp->kind) {
    case MAP_ELASTIC: return rec ? debig_hip_png_elastic_color_batch(src, out, (const debig_png_elastic_color_task *)t, w, w, cnt, NULL)
                                 : debig_hip_png_elastic_batch(src, out, (const debig_png_elastic_task *)t, w, cnt, NULL);
    case MAP_PERSP: return rec ? debig_hip_png_persp_color_batch(src, out, (const debig_png_persp_color_task *)t, w, cnt, NULL)
                               : debig_hip_png_persp_batch(src, out, (const debig_png_persp_task *)t, cnt, NULL);
    default: return rec ? debig_hip_png_warp_color_batch(src, out, (const debig_png_warp_color_task *)t, w, cnt, NULL)
                        : debig_hip_png_warp_batch(src, out, (const debig_png_warp_task *)t, cnt, NULL);
    }
}

/* debig_png_decode_batch_tensor_warp (colors == NULL) and debig_png_decode_batch_tensor_warp_color behind their argument checks.
 * With colors the tasks are debig_png_warp_color_task -- the warp task and the place of the image's record, which travels as the
 * launch's one table -- and go to the colour kernel.  tp != NULL (debig_png_decode_batch_tensor_tone, _blur): as in tensor_core, the
 * tasks of the tone and blur files come last, write UINT8 HWC into the tone arena through a launch of their own, and tone_run and
 * blur_run follow.  mp: the call's map, not yet prepared.  Projective (debig_png_decode_batch_tensor_persp): each task is followed
 * by its p[] and goes to the persp kernel of the same kind; nothing else differs.  Elastic (debig_png_decode_batch_tensor_elastic):
 * the elastic arguments are checked here, behind everything else; each task is followed by the place of its file's field, the
 * quantised fields are the launch's last table, and the tasks go to the elastic kernel of the same kind. */
static int tensor_warp_core(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out, const debig_png_box *boxes,
                            warp_map *mp, const debig_png_color *colors, uint32_t *status, debig_png_info *infos,
                            uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc, const debig_png_warp_desc *wd,
                            tone_plan *tp)
{
    const uint32_t fmt = desc->out_format, ch = fmt_channels(fmt), bits = fmt & DEBIG_PNG_FMT_16 ? 16u : 8u, sb = bits / 8u;
    const uint32_t W = desc->out_w, H = desc->out_h;
    const uint32_t es = desc->dtype == DEBIG_PNG_T_UINT ? sb : desc->dtype == DEBIG_PNG_T_F32 ? 4u : 2u;
    const uint64_t slot = (uint64_t)H * W * ch * es;
    const uint32_t run = row_run(W, WARP_TASK_PIXELS);
    const int ela = mp->kind == MAP_ELASTIC;

    stage S = {NULL, NULL, NULL, NULL, NULL};
    uint8_t *cbad = NULL;
    debig_png_color_rec *crec = NULL;
    map_tasks T = {NULL, 0, 0, colors ? sizeof(debig_png_warp_color_task) : sizeof(debig_png_warp_task), 0};
    T.elem = T.base + map_tail_bytes(mp);
    int rc;
    if ((rc = map_prepare(mp, n, W, H))) goto done;
    if (colors && (rc = color_prepare(colors, n, bits, &crec, &cbad))) goto done;
    if ((rc = tone_prepare(tp, n))) goto done;
    const stage_rule rule = {fmt, 0, 0, 0, 0, 0, mp->bad, cbad, tp ? tp->bad : NULL, tp ? tp->blur_bad : NULL}; /* no crop-size cap */
    if ((rc = stage_decode(&S, &rule, inputs, input_sizes, boxes, status, infos, n, flags))) goto done;
    if ((rc = tone_place(tp, status, n, W, H))) goto done;
    /* the plain warp has no tables (the six int64 travel in the task); with colours the records are the first table, at offset 0;
     * the tone call's tables follow; the fields come last */
    dev_table tab[3] = {{crec, colors ? (uint64_t)n * sizeof *crec : 0, 0}, {tp ? tp->lut : NULL, tone_table_bytes(tp), 0}, {NULL, 0, 0}};
    const uint32_t n_tab = (tp ? 2u : 1u) + (ela ? 1u : 0u);
    if (ela && !tp) tab[1] = tab[2];
    dev_tables_place(tab, n_tab);
    map_place(mp, &tab[n_tab - 1], n);
    const uint64_t lut_off = tp ? tone_fill(tp, n, tab[1].off) : 0;
    uint64_t n_direct = 0; /* with tp: the tasks in front of those of the tone files */
    rc = 2;
    for (uint64_t q = 0; q < (tp ? 2u : 1u) * (uint64_t)n; q++) { /* (with tp: every file twice, the tone files the second time) */
        const uint32_t pass = q >= n, i = (uint32_t)(pass ? q - n : q);
        if (q == n) n_direct = T.n;
        if (status[i] != DEBIG_PNG_OK || tone_is(tp, i) != (int)pass) continue;
        debig_png_warp_color_task p; /* (the plain task: its first `base` bytes) */
        memset(&p, 0, sizeof p);
        p.color_off = (uint64_t)i * sizeof *crec;
        p.src_off = S.offs[i] + ((uint64_t)S.box[i].y * S.inf[i].width + S.box[i].x) * ch * sb;
        p.out_off = (uint64_t)i * slot;
        memcpy(p.m, mp->m + MAP_INTS * (size_t)i, sizeof p.m);
        p.src_pitch = S.inf[i].width * ch;
        p.crop_w = S.box[i].w;
        p.crop_h = S.box[i].h;
        p.out_w = W;
        p.out_h = H;
        p.out_sx = desc->out_layout == DEBIG_PNG_LAYOUT_CHW ? 1u : ch;
        p.out_sy = desc->out_layout == DEBIG_PNG_LAYOUT_CHW ? W : W * ch;
        p.out_sc = desc->out_layout == DEBIG_PNG_LAYOUT_CHW ? H * W : 1u;
        p.channels = (uint8_t)ch;
        p.bits = (uint8_t)bits;
        p.dtype = (uint8_t)desc->dtype;
        p.filter = (uint8_t)wd->filter;
        p.border_mode = (uint8_t)wd->border_mode;
        for (uint32_t k = 0; k < 4; k++) {
            p.border[k] = k < ch ? wd->border[k] : 0;
            p.a[k] = (float)((double)desc->scale[k] / ((double)((1u << bits) - 1u) * (double)(1u << (30u - bits))));
            p.b[k] = desc->bias[k];
        }
        if (pass) { /* the 8-bit HWC intermediate */
            p.out_off = (uint64_t)tp->place[i] * tp->img;
            p.out_sx = ch;
            p.out_sy = W * ch;
            p.out_sc = 1u;
            p.dtype = DEBIG_PNG_T_UINT;
        }
        if (!map_task_runs(&T, mp, &p, &p.row0, &p.rows, H, run, i)) goto done;
    }
    if (!tp) n_direct = T.n;
    rc = 0;
    if (T.n == 0) goto done;
    debig_ctx *c = dev_upload(T.v, T.n, T.elem, tab, n_tab, &rc);
    if (!c) goto done;
    if (T.n > n_direct && (rc = debig_devbuf_reserve(&c->tone_px, tone_arena_bytes(tp)))) goto done;
    for (uint32_t part = 0; part < 2; part++) { /* the caller's tensor, then the tone arena */
        const uint8_t *d_tasks = (const uint8_t *)c->rsz_tasks.ptr + (part ? n_direct * T.elem : 0);
        const uint64_t cnt = part ? T.n - n_direct : n_direct;
        if (cnt == 0) continue;
        if ((rc = map_launch_image(mp, colors, c, part ? c->tone_px.ptr : d_out, d_tasks, (uint32_t)cnt))) goto done;
    }
    if ((rc = tone_run(tp, c, d_out, n, desc, lut_off)) || (rc = blur_run(tp, c, d_out, n, desc, lut_off))) goto done;
    rc = debig_hip_stream_sync(NULL);
done:
    stage_free(&S);
    tone_free(tp);
    map_release(mp);
    free(crec);
    free(cbad);
    free(T.v);
    return rc;
}

DEBIG_API int debig_png_decode_batch_tensor_warp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                 const debig_png_box *boxes, const debig_png_warp *warps, uint32_t *status,
                                                 debig_png_info *infos, uint32_t n, uint32_t flags,
                                                 const debig_png_tensor_desc *desc, const debig_png_warp_desc *wd)
{
    if (n == 0) return 0;
    const int badarg = tensor_warp_check(d_out, warps, desc, wd);
    if (badarg) return badarg;
    return tensor_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_AFFINE, .warps = warps), NULL, status, infos, n, flags, desc, wd, NULL);
}

DEBIG_API int debig_png_decode_batch_tensor_warp_color(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                       const debig_png_box *boxes, const debig_png_warp *warps,
                                                       const debig_png_color *colors, uint32_t *status, debig_png_info *infos,
                                                       uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc,
                                                       const debig_png_warp_desc *wd)
{
    /* every check of debig_png_decode_batch_tensor_warp first and unchanged, then the matrix call's own */
    if (n == 0) return 0;
    const int badarg = tensor_warp_check(d_out, warps, desc, wd);
    if (badarg) return badarg;
    if (!colors || !color_layout_ok(desc->out_format)) return DEBIG_PNG_BAD_ARG;
    return tensor_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_AFFINE, .warps = warps), colors, status, infos, n, flags, desc, wd, NULL);
}

/* which of the two calls with work behind the tensor a public entry point is: the tone call requires tones, the blur call blurs */
typedef enum post_kind { POST_TONE, POST_BLUR } post_kind;

/* debig_png_decode_batch_tensor_tone and debig_png_decode_batch_tensor_blur (post says which), under the call's map.  An affine
 * map whose warps are NULL, with wd NULL: the resize route.  A projective or elastic map: the same two calls behind
 * debig_png_decode_batch_tensor_persp and _elastic -- the map's array and wd are required, refused where the warp's are; the
 * elastic arguments are checked behind everything else (map_prepare, the first step of tensor_warp_core) */
static int tensor_post_call(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out, const debig_png_box *boxes,
                            warp_map *mp, const debig_png_color *colors, post_kind post, const debig_png_tone *tones,
                            const uint8_t *tables, uint32_t n_tables, const debig_png_blur *blurs, uint32_t *status,
                            debig_png_info *infos, uint32_t n, uint32_t flags, const debig_png_tensor_desc *desc,
                            const debig_png_alpha_desc *alpha, const debig_png_filter_desc *filter, const debig_png_warp_desc *wd)
{
    /* every check of the call that is extended first, unchanged and in its order; then the call's own */
    if (n == 0) return 0;
    uint32_t amode = DEBIG_PNG_ALPHA_STRAIGHT;
    if (map_given(mp) || wd || mp->kind != MAP_AFFINE) { /* (not affine: the map and its descriptor are required) */
        const int badarg = tensor_warp_check(d_out, map_given(mp), desc, wd);
        if (badarg) return badarg;
        if ((colors && !color_layout_ok(desc->out_format)) || alpha || filter) return DEBIG_PNG_BAD_ARG;
    } else if (colors) {
        const int badarg = tensor_args_check(d_out, desc);
        if (badarg) return badarg;
        if (filter && (filter->filter > DEBIG_PNG_FILTER_NEAREST || filter->reserved != 0)) return DEBIG_PNG_BAD_ARG;
        if (!color_layout_ok(desc->out_format) || (filter && filter->filter == DEBIG_PNG_FILTER_BICUBIC) || alpha) return DEBIG_PNG_BAD_ARG;
    } else {
        const int badarg = tensor_alpha_check(d_out, desc, alpha, &amode);
        if (badarg) return badarg;
        if (filter && (filter->filter > DEBIG_PNG_FILTER_NEAREST || filter->reserved != 0)) return DEBIG_PNG_BAD_ARG;
    }
    if ((post == POST_BLUR ? !blurs : !tones) || (desc->out_format & DEBIG_PNG_FMT_16) || amode == DEBIG_PNG_ALPHA_PREMULTIPLIED ||
        (!tables && n_tables > 0))
        return DEBIG_PNG_BAD_ARG;
    tone_plan tp;
    memset(&tp, 0, sizeof tp);
    tp.tones = tones;
    tp.tables = tables;
    tp.n_tables = n_tables;
    tp.blurs = blurs;
    tp.oc = fmt_channels(desc->out_format);
    if (map_given(mp)) return tensor_warp_core(inputs, input_sizes, d_out, boxes, mp, colors, status, infos, n, flags, desc, wd, &tp);
    return tensor_core(inputs, input_sizes, d_out, boxes, status, infos, n, flags, desc, amode, alpha ? alpha->background : NULL,
                       filter ? filter->filter : DEBIG_PNG_FILTER_BILINEAR, colors, &tp);
}

DEBIG_API int debig_png_decode_batch_tensor_tone(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                 const debig_png_box *boxes, const debig_png_warp *warps,
                                                 const debig_png_color *colors, const debig_png_tone *tones, const uint8_t *tables,
                                                 uint32_t n_tables, uint32_t *status, debig_png_info *infos, uint32_t n,
                                                 uint32_t flags, const debig_png_tensor_desc *desc,
                                                 const debig_png_alpha_desc *alpha, const debig_png_filter_desc *filter,
                                                 const debig_png_warp_desc *wd)
{
    return tensor_post_call(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_AFFINE, .warps = warps), colors, POST_TONE, tones,
                            tables, n_tables, NULL, status, infos, n, flags, desc, alpha, filter, wd);
}

DEBIG_API int debig_png_decode_batch_tensor_blur(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                 const debig_png_box *boxes, const debig_png_warp *warps,
                                                 const debig_png_color *colors, const debig_png_tone *tones, const uint8_t *tables,
                                                 uint32_t n_tables, const debig_png_blur *blurs, uint32_t *status,
                                                 debig_png_info *infos, uint32_t n, uint32_t flags,
                                                 const debig_png_tensor_desc *desc, const debig_png_alpha_desc *alpha,
                                                 const debig_png_filter_desc *filter, const debig_png_warp_desc *wd)
{
    return tensor_post_call(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_AFFINE, .warps = warps), colors, POST_BLUR, tones,
                            tables, n_tables, blurs, status, infos, n, flags, desc, alpha, filter, wd);
}

/* debig_png_decode_batch_tensor_persp and _elastic behind the making of their map: the affine call that the given arguments name,
 * its checks in its order: _tensor_blur with blurs, _tensor_tone with tones, else _tensor_warp_color or _tensor_warp; then the
 * map's own arguments (map_prepare) */
static int tensor_map_call(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out, const debig_png_box *boxes,
                           warp_map *mp, const debig_png_color *colors, const debig_png_tone *tones, const uint8_t *tables,
                           uint32_t n_tables, const debig_png_blur *blurs, uint32_t *status, debig_png_info *infos, uint32_t n,
                           uint32_t flags, const debig_png_tensor_desc *desc, const debig_png_warp_desc *wd)
{
    if (tones || blurs)
        return tensor_post_call(inputs, input_sizes, d_out, boxes, mp, colors, blurs ? POST_BLUR : POST_TONE, tones, tables, n_tables,
                                blurs, status, infos, n, flags, desc, NULL, NULL, wd);
    if (n == 0) return 0;
    const int badarg = tensor_warp_check(d_out, map_given(mp), desc, wd);
    if (badarg) return badarg;
    if (colors && !color_layout_ok(desc->out_format)) return DEBIG_PNG_BAD_ARG;
    return tensor_warp_core(inputs, input_sizes, d_out, boxes, mp, colors, status, infos, n, flags, desc, wd, NULL);
}

DEBIG_API int debig_png_decode_batch_tensor_persp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                  const debig_png_box *boxes, const debig_png_persp *persps,
                                                  const debig_png_color *colors, const debig_png_tone *tones, const uint8_t *tables,
                                                  uint32_t n_tables, const debig_png_blur *blurs, uint32_t *status,
                                                  debig_png_info *infos, uint32_t n, uint32_t flags,
                                                  const debig_png_tensor_desc *desc, const debig_png_warp_desc *wd)
{
    return tensor_map_call(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_PERSP, .persps = persps), colors, tones, tables,
                           n_tables, blurs, status, infos, n, flags, desc, wd);
}

DEBIG_API int debig_png_decode_batch_tensor_elastic(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                    const debig_png_box *boxes, const debig_png_warp *warps,
                                                    const debig_png_color *colors, const debig_png_tone *tones, const uint8_t *tables,
                                                    uint32_t n_tables, const debig_png_blur *blurs, uint32_t *status,
                                                    debig_png_info *infos, uint32_t n, uint32_t flags,
                                                    const debig_png_tensor_desc *desc, const debig_png_warp_desc *wd,
                                                    const debig_png_elastic *elastics, const debig_png_elastic_desc *ed)
{
    return tensor_map_call(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_ELASTIC, .warps = warps, .elastics = elastics, .ed = ed), colors, tones, tables,
                           n_tables, blurs, status, infos, n, flags, desc, wd);
}

/* the warp arguments of the two label calls, behind the checks of the call without a warp: the map's array, wd, the border mode,
 * and a CONSTANT border label that the dtype holds -> 0 or DEBIG_PNG_BAD_ARG */
static int label_warp_check(const warp_map *mp, const debig_png_label_warp_desc *wd, uint32_t dtype)
{
    if (!map_given(mp) || !wd || wd->border_mode > DEBIG_PNG_BORDER_CLAMP) return DEBIG_PNG_BAD_ARG;
    if (wd->border_mode == DEBIG_PNG_BORDER_CONSTANT && dtype <= DEBIG_PNG_L_U16 &&
        (wd->border_label < 0 || wd->border_label > (dtype == DEBIG_PNG_L_U8 ? 255 : 65535)))
        return DEBIG_PNG_BAD_ARG;
    return 0;
}

/* the launch of the label kind under the call's map */
static int map_launch_labels(const warp_map *mp, const debig_ctx *c, void *d_out, const int32_t *d_lut, uint32_t cnt)
{
    const uint8_t *src = c->rsz_src.ptr, *w = c->rsz_weights.ptr;
    const void *t = c->rsz_tasks.ptr;
    switch (mp->kind) {
    case MAP_ELASTIC: return debig_hip_png_label_elastic_batch(src, d_out, (const debig_png_label_elastic_task *)t, d_lut, w, cnt, NULL);
    case MAP_PERSP: return debig_hip_png_label_persp_batch(src, d_out, (const debig_png_label_persp_task *)t, d_lut, cnt, NULL);
    default: return debig_hip_png_label_warp_batch(src, d_out, (const debig_png_label_warp_task *)t, d_lut, cnt, NULL);
    }
}

/* debig_png_decode_batch_labels_warp, _labels_persp and _labels_elastic under their map (not yet prepared); the elastic
 * arguments are checked behind the warp's */
static int labels_warp_core(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out, const debig_png_box *boxes,
                            warp_map *mp, uint32_t *status, debig_png_info *infos, uint32_t n, uint32_t flags,
                            const debig_png_label_desc *desc, const debig_png_label_warp_desc *wd)
{
    /* every check of debig_png_decode_batch_labels first and unchanged, then the warp's; all before any file is looked at */
    if (n == 0) return 0;
    const int badarg = label_args_check(d_out, desc);
    if (badarg) return badarg;
    if (label_warp_check(mp, wd, desc->dtype)) return DEBIG_PNG_BAD_ARG;
    const uint32_t W = desc->out_w, H = desc->out_h, es = 1u << desc->dtype;
    const uint32_t run = row_run(W, WARP_TASK_PIXELS);

    stage S = {NULL, NULL, NULL, NULL, NULL};
    map_tasks T = {NULL, 0, 0, sizeof(debig_png_label_warp_task), sizeof(debig_png_label_warp_task) + map_tail_bytes(mp)};
    int rc;
    if ((rc = map_prepare(mp, n, W, H))) goto done;
    dev_table tab[2] = {{desc->lut, 1024, 0}, {NULL, 0, 0}}; /* the LUT (or its room), the fields */
    const uint32_t n_tab = mp->kind == MAP_ELASTIC ? 2u : 1u;
    dev_tables_place(tab, n_tab);
    map_place(mp, &tab[1], n);
    /* E_LABEL: colour type 2, 4 or 6; a 16-bit file with dtype U8 or with a lut */
    const stage_rule rule = {DEBIG_PNG_FMT_GRAY | DEBIG_PNG_FMT_NATIVE_DEPTH, 1, 1, desc->dtype == DEBIG_PNG_L_U8 || desc->lut, 0, 0, mp->bad, NULL, NULL, NULL};
    if ((rc = stage_decode(&S, &rule, inputs, input_sizes, boxes, status, infos, n, flags))) goto done;
    rc = 2;
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] != DEBIG_PNG_OK) continue;
        debig_png_label_warp_task p;
        memset(&p, 0, sizeof p);
        p.src_bytes = S.inf[i].bit_depth == 16 ? 2u : 1u;
        p.src_off = S.offs[i] + ((uint64_t)S.box[i].y * S.inf[i].width + S.box[i].x) * p.src_bytes;
        p.out_off = (uint64_t)i * H * W * es;
        memcpy(p.m, mp->m + MAP_INTS * (size_t)i, sizeof p.m);
        p.src_pitch = S.inf[i].width;
        p.crop_w = S.box[i].w;
        p.crop_h = S.box[i].h;
        p.out_w = W;
        p.out_h = H;
        p.border_label = wd->border_label;
        p.dtype = (uint8_t)desc->dtype;
        p.border_mode = (uint8_t)wd->border_mode;
        if (!map_task_runs(&T, mp, &p, &p.row0, &p.rows, H, run, i)) goto done;
    }
    rc = 0;
    if (T.n == 0) goto done;
    debig_ctx *c = dev_upload(T.v, T.n, T.elem, tab, n_tab, &rc);
    if (!c) goto done;
    if ((rc = map_launch_labels(mp, c, d_out, desc->lut ? (const int32_t *)c->rsz_weights.ptr : NULL, (uint32_t)T.n))) goto done;
    rc = debig_hip_stream_sync(NULL);
done:
    stage_free(&S);
    map_release(mp);
    free(T.v);
    return rc;
}

DEBIG_API int debig_png_decode_batch_labels_warp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                 const debig_png_box *boxes, const debig_png_warp *warps, uint32_t *status,
                                                 debig_png_info *infos, uint32_t n, uint32_t flags,
                                                 const debig_png_label_desc *desc, const debig_png_label_warp_desc *wd)
{
    return labels_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_AFFINE, .warps = warps), status, infos, n, flags, desc, wd);
}

DEBIG_API int debig_png_decode_batch_labels_persp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                  const debig_png_box *boxes, const debig_png_persp *persps, uint32_t *status,
                                                  debig_png_info *infos, uint32_t n, uint32_t flags,
                                                  const debig_png_label_desc *desc, const debig_png_label_warp_desc *wd)
{
    return labels_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_PERSP, .persps = persps), status, infos, n, flags, desc, wd);
}

DEBIG_API int debig_png_decode_batch_labels_elastic(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                    const debig_png_box *boxes, const debig_png_warp *warps, uint32_t *status,
                                                    debig_png_info *infos, uint32_t n, uint32_t flags,
                                                    const debig_png_label_desc *desc, const debig_png_label_warp_desc *wd,
                                                    const debig_png_elastic *elastics, const debig_png_elastic_desc *ed)
{
    return labels_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_ELASTIC, .warps = warps, .elastics = elastics, .ed = ed), status,
                            infos, n, flags, desc, wd);
}

/* the launch of the colour-label kind under the call's map; the maps' tables are the first table of the launch */
static int map_launch_color_labels(const warp_map *mp, const debig_ctx *c, void *d_out, uint32_t *d_cnt, uint32_t cnt)
{
    const uint8_t *src = c->rsz_src.ptr, *w = c->rsz_weights.ptr;
    const void *t = c->rsz_tasks.ptr;
    switch (mp->kind) {
    case MAP_ELASTIC: return debig_hip_png_color_label_elastic_batch(src, d_out, (const debig_png_color_label_elastic_task *)t, w, d_cnt, w, cnt, NULL);
    case MAP_PERSP: return debig_hip_png_color_label_persp_batch(src, d_out, (const debig_png_color_label_persp_task *)t, w, d_cnt, cnt, NULL);
    default: return debig_hip_png_color_label_warp_batch(src, d_out, (const debig_png_color_label_warp_task *)t, w, d_cnt, cnt, NULL);
    }
}

/* debig_png_decode_batch_color_labels_warp, _color_labels_persp and _color_labels_elastic under their map (not yet prepared); the
 * elastic arguments are checked behind the warp's */
static int color_labels_warp_core(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out, const debig_png_box *boxes,
                                  warp_map *mp, uint32_t *status, debig_png_info *infos, uint32_t *unmatched, uint32_t n,
                                  uint32_t flags, const debig_png_color_label_desc *desc, const debig_png_label_warp_desc *wd)
{
    /* every check of debig_png_decode_batch_color_labels first and unchanged, then the warp's; all before any file is looked at */
    if (n == 0) return 0;
    clbl_maps M = {NULL, NULL, 0, NULL};
    uint32_t *cnt = NULL;
    stage S = {NULL, NULL, NULL, NULL, NULL};
    map_tasks T = {NULL, 0, 0, sizeof(debig_png_color_label_warp_task), sizeof(debig_png_color_label_warp_task) + map_tail_bytes(mp)};
    int rc;
    if ((rc = clbl_args_check(d_out, desc, n, &M))) goto done;
    if ((rc = label_warp_check(mp, wd, desc->dtype))) goto done;
    const int map_mode = desc->mode == DEBIG_PNG_CL_MAP;
    const uint32_t W = desc->out_w, H = desc->out_h, es = 1u << desc->dtype, n_maps = map_mode ? desc->n_maps : 0;
    const uint32_t run = row_run(W, WARP_TASK_PIXELS);
    /* the maps' tables (first: map_off needs no base), the counters (16-byte aligned: a table is a multiple of 16 bytes) */
    dev_table tab[3] = {{M.tab, M.bytes, 0}, {NULL, (uint64_t)n * sizeof(uint32_t), 0}, {NULL, 0, 0}}; /* (the fields come last) */
    const uint32_t n_tab = mp->kind == MAP_ELASTIC ? 3u : 2u;
    if ((rc = map_prepare(mp, n, W, H))) goto done;
    rc = 2;
    cnt = (uint32_t *)calloc(n, sizeof(uint32_t));
    if (!cnt) goto done;
    const stage_rule rule = {DEBIG_PNG_FMT_RGB | DEBIG_PNG_FMT_8, 0, 0, 1, 0, 0, mp->bad, NULL, NULL, NULL}; /* E_LABEL: a 16-bit file */
    if ((rc = stage_decode(&S, &rule, inputs, input_sizes, boxes, status, infos, n, flags))) goto done;
    if (unmatched) memset(unmatched, 0, (size_t)n * sizeof(uint32_t));
    dev_tables_place(tab, n_tab);
    map_place(mp, &tab[2], n);
    rc = 2;
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] != DEBIG_PNG_OK) continue;
        const uint32_t mk = n_maps == 1 ? 0u : i;
        debig_png_color_label_warp_task p;
        memset(&p, 0, sizeof p);
        p.src_off = S.offs[i] + ((uint64_t)S.box[i].y * S.inf[i].width + S.box[i].x) * 3u;
        p.out_off = (uint64_t)i * H * W * es;
        memcpy(p.m, mp->m + MAP_INTS * (size_t)i, sizeof p.m);
        p.src_pitch = S.inf[i].width;
        p.crop_w = S.box[i].w;
        p.crop_h = S.box[i].h;
        p.out_w = W;
        p.out_h = H;
        p.border_label = wd->border_label;
        p.dtype = (uint8_t)desc->dtype;
        p.mode = (uint8_t)desc->mode;
        p.border_mode = (uint8_t)wd->border_mode;
        p.image = i;
        if (map_mode) {
            p.map_off = tab[0].off + M.off[mk];
            p.map_slots = M.slots[mk];
            p.missing = desc->missing;
        }
        if (!map_task_runs(&T, mp, &p, &p.row0, &p.rows, H, run, i)) goto done;
    }
    rc = 0;
    if (T.n == 0) goto done;
    debig_ctx *c = dev_upload(T.v, T.n, T.elem, tab, n_tab, &rc);
    if (!c) goto done;
    uint32_t *d_cnt = map_mode ? (uint32_t *)((uint8_t *)c->rsz_weights.ptr + tab[1].off) : NULL;
    if ((d_cnt && (rc = debig_hip_memset(d_cnt, 0, tab[1].bytes, NULL))) ||
        (rc = map_launch_color_labels(mp, c, d_out, d_cnt, (uint32_t)T.n)) ||
        (d_cnt && (rc = debig_hip_memcpy_d2h(cnt, d_cnt, tab[1].bytes, NULL))) ||
        (rc = debig_hip_stream_sync(NULL)))
        goto done;
    if (unmatched && map_mode) memcpy(unmatched, cnt, (size_t)n * sizeof(uint32_t));
done:
    clbl_maps_free(&M);
    free(cnt);
    stage_free(&S);
    map_release(mp);
    free(T.v);
    return rc;
}

DEBIG_API int debig_png_decode_batch_color_labels_warp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                       const debig_png_box *boxes, const debig_png_warp *warps, uint32_t *status,
                                                       debig_png_info *infos, uint32_t *unmatched, uint32_t n, uint32_t flags,
                                                       const debig_png_color_label_desc *desc,
                                                       const debig_png_label_warp_desc *wd)
{
    return color_labels_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_AFFINE, .warps = warps), status, infos,
                                  unmatched, n, flags, desc, wd);
}

DEBIG_API int debig_png_decode_batch_color_labels_persp(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                        const debig_png_box *boxes, const debig_png_persp *persps, uint32_t *status,
                                                        debig_png_info *infos, uint32_t *unmatched, uint32_t n, uint32_t flags,
                                                        const debig_png_color_label_desc *desc,
                                                        const debig_png_label_warp_desc *wd)
{
    return color_labels_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_PERSP, .persps = persps), status, infos,
                                  unmatched, n, flags, desc, wd);
}

DEBIG_API int debig_png_decode_batch_color_labels_elastic(const uint8_t *const *inputs, const uint64_t *input_sizes, void *d_out,
                                                          const debig_png_box *boxes, const debig_png_warp *warps, uint32_t *status,
                                                          debig_png_info *infos, uint32_t *unmatched, uint32_t n, uint32_t flags,
                                                          const debig_png_color_label_desc *desc,
                                                          const debig_png_label_warp_desc *wd, const debig_png_elastic *elastics,
                                                          const debig_png_elastic_desc *ed)
{
    return color_labels_warp_core(inputs, input_sizes, d_out, boxes, MAP_OF(MAP_ELASTIC, .warps = warps, .elastics = elastics, .ed = ed), status, infos,
                                  unmatched, n, flags, desc, wd);
}
