/* Internal (host side, plain C): the chunk walk of debig_png_spec.c and the helpers its decode shares with the APNG
 * decode (debig_apng.c). */
#ifndef DEBIG_PNG_SPEC_H
#define DEBIG_PNG_SPEC_H
#include <stdint.h>
#include <stddef.h>
#include "decode_png.h"
#include "debig_ctx.h"

typedef struct spec_piece { uint64_t off, len; } spec_piece;
typedef struct spec_chunk { uint64_t off, len; uint32_t crc; } spec_chunk;

typedef struct spec_file {
    uint32_t status;
    debig_png_info info;
    uint32_t n_chunks, cap_chunks, n_idat, cap_idat;
    spec_chunk *chunks; /* type + data spans and the CRCs stored in the file */
    spec_piece *idat;   /* IDAT payloads, in file order */
    uint64_t z_total;   /* bytes of the concatenated IDAT payloads (zlib header + DEFLATE + trailer) */
    uint32_t pal[256];  /* RGBA, tRNS alpha folded in */
    uint32_t n_pal;
    uint16_t key[3];
    uint32_t has_key, general;
    uint32_t planar;    /* channel planes (c, y, x) instead of interleaved pixels: the planar de-filter kernel */
    uint32_t fmt;       /* resolved output format: layout (0..3) | DEBIG_PNG_FMT_16, 0 = RGBA8 */
    uint64_t out_bytes; /* bytes of the output in that format */
    uint64_t scan;      /* scanline stream bytes */
    /* device layout */
    uint64_t file_off, in_off, out_off, pal_off, scratch_off, rgba_off;
} spec_file;

/* The chunk walk.  info_only: stop at the first IDAT (debig_png_info_get).  Returns a DEBIG_PNG_* status. */
uint32_t spec_walk(const uint8_t *in, uint64_t size, spec_file *F, int info_only);
void spec_free(spec_file *F);
int spec_grow(void **p, uint32_t *cap, uint32_t n, size_t elem);
uint32_t spec_be32(const uint8_t *p);
/* the two zlib header bytes pass: CM = 8, CINFO <= 7, FCHECK, no FDICT */
int spec_zlib_header_ok(uint32_t cmf, uint32_t flg);
/* scanline stream bytes of a w x h image with info's colour type, depth and interlace */
uint64_t spec_scan_bytes(const debig_png_info *info, uint32_t w, uint32_t h);
/* 1: the image goes through the general de-filter kernel, 0: through the tuned ones (decode_png.h: routing) */
int spec_is_general(const spec_file *F, uint32_t flags);
/* the general-kernel tasks of a w x h image (*n_tasks) and the scratch they need, in bytes */
uint64_t spec_general_scratch(const debig_png_info *info, uint32_t w, uint32_t h, uint32_t *n_tasks);
/* the general-kernel tasks of a w x h image with F's colour type, depth, interlace, palette (at F->pal_off), tRNS key
 * and output format; its scanline stream at stream_off, its pixels at rgba_off.  Written to t[0..), their number returned */
uint32_t spec_image_tasks(const spec_file *F, uint32_t w, uint32_t h, uint64_t stream_off, uint64_t rgba_off,
                          uint64_t scratch_off, debig_png_spec_task *t);

#endif
